"""The carried Flock rollout (env_rollout_w64 with CARRY, csrc/flock_step_w64.hip): between the steps of
one launch a wave keeps its env's state, the first two list chunks and the next step's actions in
registers, and waits for its stores only before a step that has to load (the first step of a launch,
after a spill step, a raised status bit, or a list longer than the two register chunks).

The bar: a carried value is bit for bit what the load would return. Every case compares state
(get_state), outputs, counters and reward sums bitwise against K step() calls on a twin world, and
against the same rollout with MACM_DEBUG_ROLLOUT_RELOAD set (every step loads and fences)."""
import numpy as np
import pytest
import torch

from test_gpu_rollout import assert_same, flock_actions
from test_gpu_trajectory import assert_traj, per_step

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

RCH_ENTRIES = 128  # RCH * W of flock_step_w64.hip: the list entries a wave keeps in registers


def triple(E, n_agents, seed, **kw):
    """(per-step twin, carried rollout, rollout that reloads every step)"""
    a, b, c = (FlockVec(E, n_agents=n_agents, seed=seed, device="cuda:0", **kw) for _ in range(3))
    c.world.set_debug(_abi.DEBUG_ROLLOUT_RELOAD)
    return a, b, c


def assert_all(a, b, c, ctx):
    for v, nm in ((b, "carried"), (c, "reload")):
        assert_same(a, v, f"{ctx} ({nm})")
        pa, ta = a.reward_sums()
        pv, tv = v.reward_sums()
        np.testing.assert_array_equal(pa, pv, err_msg=f"{ctx} ({nm}): reward sums")
        assert ta == tv, f"{ctx} ({nm}): reward total"
        assert v.status() == 0


def run_both_forms(a, b, c, acts, trajectory, ctx):
    if trajectory:  # row k of every output is step k's
        ref = per_step(a, acts)
        assert_traj(ref, b.rollout(acts, trajectory=True), f"{ctx} (carried)")
        assert_traj(ref, c.rollout(acts, trajectory=True), f"{ctx} (reload)")
    else:
        for k in range(acts.shape[0]):
            a.step(acts[k])
        b.rollout(acts)
        c.rollout(acts)
    assert_all(a, b, c, ctx)


@pytest.mark.parametrize("trajectory", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_short_rollouts(K, trajectory):
    """K = 1: the first step loads and the last step prefetches nothing, in one step; 2 and 3: both
    list parities; 8: a run of carried steps."""
    a, b, c = triple(8, [64], 5)
    run_both_forms(a, b, c, flock_actions(K, 8, 64, 11), trajectory, f"K = {K}")


@pytest.mark.parametrize("E,n_agents,kw", [
    (16, [20], {}),                                      # the 32-lane instantiation, lanes >= N
    (8, [64], {"obs_dtype": torch.float64}),
    (12, [30], {"action_mode": "continuous"}),           # the action prefetch's other width
    (8, [16, 16, 16, 16], {"targets": [i // 16 for i in range(64)]}),  # 4 flocks: a target per lane
])
@pytest.mark.parametrize("trajectory", [False, True])
def test_instantiations(E, n_agents, kw, trajectory):
    K, N = 6, sum(n_agents)
    a, b, c = triple(E, n_agents, 7, **kw)
    acts = flock_actions(K, E, N, 3, kw.get("action_mode") == "continuous")
    run_both_forms(a, b, c, acts, trajectory, f"{n_agents} {kw}")


def test_actions_of_exactly_k_rows_at_the_end_of_a_buffer():
    """The last step must not load a row K: the actions are the tail of their tensor."""
    E, N, K = 8, 64, 5
    a, b, c = triple(E, [N], 9)
    big = torch.zeros((K + 3, E, N, 3), dtype=torch.uint8, device="cuda:0")
    big[3:] = flock_actions(K, E, N, 19)
    acts = big[3:]
    assert acts.data_ptr() + acts.numel() == big.data_ptr() + big.numel()
    run_both_forms(a, b, c, acts, False, "tail view")
    run_both_forms(a, b, c, acts, True, "tail view, trajectory")


@pytest.mark.parametrize("trajectory", [False, True])
def test_list_grows_beyond_the_register_chunks_and_shrinks_again(trajectory):
    """N = 64 at start_spread 10, seed 6 (chosen with the CPU oracle): env 2's list has 95 entries at the
    start, 126 after step 0, 131 after step 1 and 128 again after step 4; env 0's falls from 129 to 127
    in step 10. One launch of 16 steps, so these crossings are inside it: a carried step ends with a
    list above 128 entries (fence, the next step loads every chunk) and a loading step with at most
    128 (the next step is carried again). Shown by the device's own list counts, read from the
    per-step twin after every step (the rollouts' state is asserted equal to the twin's)."""
    E, N, K = 4, 64, 16
    a, b, c = triple(E, [N], 6, start_spread=10)
    rng = np.random.default_rng(6)
    acts = torch.from_numpy(np.stack([rng.integers(0, 3, size=(E, N, 3)).astype(np.uint8)
                                      for _ in range(K)])).cuda()
    cnt = [a.get_state()["contact_count"].copy()]  # cnt[k + 1]: the lists after step k
    rows = {k: [] for k in ("obs", "nbr_id", "reward", "collided", "done")}
    for k in range(K):
        a.step(acts[k])
        cnt.append(a.get_state()["contact_count"].copy())
        for key in rows:
            rows[key].append(getattr(a.world, key).clone())
    if trajectory:
        ref = {k: torch.stack(v) for k, v in rows.items()}
        assert_traj(ref, b.rollout(acts, trajectory=True), "long lists (carried)")
        assert_traj(ref, c.rollout(acts, trajectory=True), "long lists (reload)")
    else:
        b.rollout(acts)
        c.rollout(acts)
    assert_all(a, b, c, "long lists")
    cnt = np.array(cnt)
    # steps 1 .. K - 2: not the launch's first (which loads anyway) and with a step after them
    grew = [(k, e) for k in range(1, K - 1) for e in range(E)
            if cnt[k, e] <= RCH_ENTRIES < cnt[k + 1, e]]
    shrank = [(k, e) for k in range(1, K - 1) for e in range(E)
              if cnt[k, e] > RCH_ENTRIES >= cnt[k + 1, e]]
    assert grew and shrank, cnt
    assert b.spilled() == 0


@pytest.mark.parametrize("trajectory", [False, True])
def test_spill_step_in_the_middle_of_a_rollout(trajectory):
    """Dense start (start_spread 4): some env-steps take the spill step and some do not, so a carried
    run hands over to the spill step (after waiting for its stores) and the steps after it load."""
    E, N, K = 8, 64, 12
    a, b, c = triple(E, [N], 5, start_spread=4)
    s0 = b.spilled()
    run_both_forms(a, b, c, flock_actions(K, E, N, 11), trajectory, "dense")
    assert 0 < b.spilled() - s0 < E * K, b.spilled() - s0
    assert a.spilled() == b.spilled() == c.spilled()


def test_continuation_and_injected_state():
    """Global memory is complete after a carried launch: a step and a second rollout stay in lockstep
    with the per-step twin; a rollout after set_state starts from the injected state."""
    E, N, K = 8, 64, 5
    a, b, c = triple(E, [N], 13)
    acts = flock_actions(2 * K + 1, E, N, 21)
    run_both_forms(a, b, c, acts[:K], False, "first rollout")
    for v in (a, b, c):
        v.step(acts[K])
    assert_all(a, b, c, "after a step")
    run_both_forms(a, b, c, acts[K + 1:], False, "second rollout")
    d = FlockVec(E, n_agents=[N], seed=99, device="cuda:0")
    for k in range(3):
        d.step(acts[k])
    st = d.get_state()
    for v in (a, b, c):
        v.set_state(st)
    run_both_forms(a, b, c, acts[:K], True, "after set_state")
    sb = b.get_state()
    assert int(sb["step_count"][0]) == int(st["step_count"][0]) + K


def test_balanced_launch():
    """K >= 32 (kRollBalanceMinSteps): wave b steps env order[b]."""
    E, N, K = 64, 64, 33
    a, b, c = triple(E, [N], 17, start_spread=6)
    run_both_forms(a, b, c, flock_actions(K, E, N, 23), False, "balanced")
