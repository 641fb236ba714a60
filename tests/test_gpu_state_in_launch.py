"""State write-back only where something reads it (step_w64_body's wb, csrc/flock_step_w64.hip): a
carried Flock rollout step that another carried step follows stores its outputs only; the env's
state rows, its list and lane 0's per-env words stay in registers and LDS (StepCarry, EnvCarry) and
reach global memory with the launch's last step, before a step that loads (the list outgrew the
register chunks, a status bit, MACM_DEBUG_ROLLOUT_RELOAD) and at an episode's end.

The bar: global memory after a launch is what one-step launches leave. After one K-step rollout,
get_state() (positions, velocities, angles, fat AABBs, sleep times, the ordered list with impulses
and count, time_passed, step_count), the counters, the status and the reward sums are bit for bit
those of K step() calls on a twin world, as is every trajectory row. 6 envs x 64 agents and
5 envs x 40 agents (lanes >= N), K = 1 (the only step loads and writes back), 2 and 7 (both list
parities, a run of steps that store nothing but outputs)."""
import numpy as np
import pytest
import torch

from parity import oracle_for
from test_gpu_rollout import assert_same, flock_actions
from test_gpu_rollout_autoreset import assert_flock_end, flock_loop, flock_twins
from test_gpu_trajectory import assert_traj, per_step

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

RCH_ENTRIES = 128  # RCH * W of flock_step_w64.hip: the list entries a wave keeps in registers
SHAPES = [(6, 64), (5, 40)]
KS = [1, 2, 7]
shapes = pytest.mark.parametrize("E,N", SHAPES, ids=[f"{e}x{n}" for e, n in SHAPES])
steps = pytest.mark.parametrize("K", KS)


def twins(E, N, seed, n=2, **kw):
    return [FlockVec(E, n_agents=[N], seed=seed, device="cuda:0", **kw) for _ in range(n)]


def numpy_actions(K, E, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 3, size=(E, N, 3)).astype(np.uint8) for _ in range(K)])


def assert_end(a, b, ctx, status=0):
    """State, current outputs and counters (assert_same), reward sums, spilled, status."""
    assert_same(a, b, ctx)
    pa, ta = a.reward_sums()
    pb, tb = b.reward_sums()
    np.testing.assert_array_equal(pa, pb, err_msg=f"{ctx}: reward sums")
    assert ta == tb, f"{ctx}: reward total"
    assert a.spilled() == b.spilled(), f"{ctx}: spilled"
    assert a.status() == status and b.status() == status, f"{ctx}: status {a.status()}, {b.status()}"


def rollout_against_steps(a, b, acts, ctx):
    """b: one trajectory rollout; a: a step() per row. Every row, then everything after the launch."""
    assert_traj(per_step(a, acts), b.rollout(acts, trajectory=True), ctx)
    assert_end(a, b, ctx)


def oracle_list_lengths(E, N, seed, acts, **kw):
    """[K + 1, E]: the CPU oracle's list lengths before step 0 and after every step."""
    orc = oracle_for(to_config(flockSettings(**kw), N, 1, obs_f64=True), np.zeros(N, np.int32), E, seed)
    C = N * (N - 1) // 2
    cnt = [orc.get_state(C)["contact_count"].copy()]
    for k in range(acts.shape[0]):
        orc.step(acts[k])
        cnt.append(orc.get_state(C)["contact_count"].copy())
    return np.array(cnt)


@shapes
@steps
def test_default_spread(E, N, K):
    """Carried steps and a final write-back."""
    a, b = twins(E, N, 5)
    rollout_against_steps(a, b, flock_actions(K, E, N, 11), f"{E}x{N} K = {K}")
    assert int(b.get_state()["contact_count"].max()) <= RCH_ENTRIES  # every step but the first was carried


# start_spread 9 and 6 are tools/rollout_dense.py's dense worlds; seeds chosen with the CPU oracle
DENSE = {(6, 64): dict(start_spread=9, seed=1), (5, 40): dict(start_spread=6, seed=3)}


@shapes
@steps
def test_dense_start_drops_the_carry(E, N, K):
    """Lists that cross 128 entries inside the launch: the step that ends above it writes back and
    the next one loads. 6 x 64 at start_spread 9: five envs cross in step 0 (the steps after it all
    load); 5 x 40 at start_spread 6: env 4 grows from 126 to 129 entries in step 1, a carried step,
    and falls from 130 to 127 in step 5, after which the carry resumes. Precondition from the
    oracle's list lengths over 7 steps (the shorter launches run a prefix of the same actions)."""
    kw = dict(start_spread=DENSE[E, N]["start_spread"])
    seed = DENSE[E, N]["seed"]
    acts = numpy_actions(7, E, N, seed)
    cnt = oracle_list_lengths(E, N, seed, acts, **kw)
    up = [(k, e) for k in range(7) for e in range(E) if cnt[k, e] <= RCH_ENTRIES < cnt[k + 1, e]]
    assert up, cnt
    if N == 40:
        assert any(k >= 1 for k, _ in up), cnt  # a carried step (not the launch's first) outgrows the chunks
        assert any(cnt[k, e] > RCH_ENTRIES >= cnt[k + 1, e] for k in range(1, 7) for e in range(E)), cnt
    a, b = twins(E, N, seed, **kw)
    rollout_against_steps(a, b, torch.from_numpy(acts[:K]).cuda(), f"dense {E}x{N} K = {K}")
    np.testing.assert_array_equal(b.get_state()["contact_count"], cnt[K])


@shapes
@steps
def test_forced_spill_then_carried(E, N, K):
    """MACM_DEBUG_FORCE_SPILL holds for a launch: its first step, a loading one, takes the spill step
    and ends the carry, so every step of it does (a carried step never needs the spill step, which
    reads global memory). Then the switch is cleared and a carried launch continues from what the
    spill steps left."""
    a, b = twins(E, N, 7)
    acts = flock_actions(2 * K, E, N, 13)
    for v in (a, b):
        v.world.set_debug(_abi.DEBUG_FORCE_SPILL)
    rollout_against_steps(a, b, acts[:K], "forced spill")
    assert b.spilled() == E * K
    for v in (a, b):
        v.world.set_debug(0)
    rollout_against_steps(a, b, acts[K:], "carried after the spill steps")
    assert b.spilled() == E * K


# (start_spread, seed, max_contacts): the oracle's longest list is max_contacts + 1 after step 1
OVERFLOW = {(6, 64): (12, 1, 104), (5, 40): (10, 2, 55)}


@shapes
@steps
def test_contact_overflow_mid_launch(E, N, K):
    """A small max_contacts: the list of one env outgrows it in step 1 (a carried step when K = 7).
    MACM_ST_CONTACT_OVERFLOW is reported, not a fault: that step writes back and ends the carry, and
    the launch's remaining steps run on the truncated list. Step() refuses after the overflow, so
    the twin here is the same rollout with MACM_DEBUG_ROLLOUT_RELOAD (every step loads and writes
    back: a one-step launch's loads and stores); the per-step twin covers the rows up to the
    overflow's. K = 1 ends before it."""
    spread, seed, C = OVERFLOW[E, N]
    acts = numpy_actions(7, E, N, seed)
    cnt = oracle_list_lengths(E, N, seed, acts, start_spread=spread)
    assert cnt[:2].max() <= C < cnt[2].max(), cnt
    a, b, c = twins(E, N, seed, n=3, start_spread=spread, max_contacts=C)
    c.world.set_debug(_abi.DEBUG_ROLLOUT_RELOAD)
    assert b.world.C == C and b.status() == 0
    acts = torch.from_numpy(acts[:K]).cuda()
    tb, tc = b.rollout(acts, trajectory=True), c.rollout(acts, trajectory=True)
    ref = per_step(a, acts[:2])  # the step that overflows still completes; the one after it would raise
    assert_traj(ref, {k: v[:2] for k, v in tb.items()}, "rows up to the overflow")
    assert_traj(tc, tb, "carried against reload")
    want = _abi.ST_CONTACT_OVERFLOW if K >= 2 else 0
    assert_end(c, b, f"overflow K = {K}", status=want)
    if K <= 2:
        assert_end(a, b, f"overflow K = {K}, per step", status=want)


@shapes
@steps
def test_linear_reward_sums(E, N, K):
    """Linear rewards: the env's float64 reward total is carried as a running sum and stored with the
    write-back; the steps' sums are added one by one in step order, as the per-step atomic adds."""
    a, b = twins(E, N, 9, reward_mode="linear")
    rollout_against_steps(a, b, flock_actions(K, E, N, 17), f"linear K = {K}")
    rollout_against_steps(a, b, flock_actions(K, E, N, 18), f"linear, second launch K = {K}")
    assert a.reward_sums()[1] != 0.0


@shapes
@steps
def test_back_to_back_launches_then_a_step(E, N, K):
    """The hand-over between launches: two rollouts (odd K: the second starts on the other list
    parity), then a step() from what the second left."""
    a, b = twins(E, N, 13)
    acts = flock_actions(2 * K + 1, E, N, 21)
    rollout_against_steps(a, b, acts[:K], "first launch")
    rollout_against_steps(a, b, acts[K:2 * K], "second launch")
    for v in (a, b):
        v.step(acts[2 * K])
    assert_end(a, b, "a step after the launches")


# K: (time_limit, launch steps that end the episode, after one step taken before the launch)
LIMITS = {1: (0.03, [0]), 2: (0.04, [1]), 7: (0.06, [2, 6])}


@shapes
@steps
def test_autoreset_episode_ends(E, N, K):
    """Autoreset on: the step that ends an episode writes back, and the in-launch reset works on
    global memory. At 60 Hz the limits end episodes after 2, 3 and 4 steps; one step is taken before
    the launch, so they end in its last step (K = 1, 2) and in its middle and last step (K = 7)."""
    limit, ends = LIMITS[K]
    off, on = flock_twins(E, N, 15, time_limit=limit)
    acts = flock_actions(K + 1, E, N, 23)
    ref0 = flock_loop(off, acts[:1])
    assert_traj(ref0, on.rollout(acts[:1], trajectory=True), "the step before")
    ref = flock_loop(off, acts[1:])
    done = ref["done"].cpu().numpy().astype(bool)
    assert [k for k in range(K) if done[k].all()] == ends and done.any(1).sum() == len(ends), done
    assert_traj(ref, on.rollout(acts[1:], trajectory=True), f"autoreset K = {K}")
    assert_flock_end(off, on, f"autoreset K = {K}")


@shapes
@steps
def test_debug_switches_give_the_same_rows(E, N, K):
    """MACM_DEBUG_ROLLOUT_RELOAD (every step loads, so every step writes back) and
    MACM_DEBUG_NEAR_PLAIN (no candidate lists) change how a launch runs, never what it leaves."""
    a, b, c, d = twins(E, N, 19, n=4)
    c.world.set_debug(_abi.DEBUG_ROLLOUT_RELOAD)
    d.world.set_debug(_abi.DEBUG_NEAR_PLAIN)
    acts = flock_actions(K, E, N, 29)
    ref = per_step(a, acts)
    for v, nm in ((b, "carried"), (c, "reload"), (d, "near plain")):
        assert_traj(ref, v.rollout(acts, trajectory=True), nm)
        assert_end(a, v, nm)
