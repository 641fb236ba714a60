"""The Flock rollout kernels' nearest neighbour from per-agent candidate lists (csrc/flock_step_w64.hip,
above near_build; the rule restated in tests/near_candidates_ref.py).

The bar: nothing changes. Trajectory rollouts long enough for several rebuilds inside a launch give,
bit for bit, every row, the final state, the counters and the reward sums of
  - the same world stepped with one env_step_w64 launch per step (the plain sweep, untouched),
  - the same rollout with MACM_DEBUG_NEAR_PLAIN (every step the plain sweep),
and equal the oracle at the suite's bar (state bitwise, neighbour ids, rewards and collided exact,
observations by obs_check). For every rollout the CPU restatement, applied to the oracle's positions,
says which kinds of step occur, so that the comparison is not of plain against plain."""
import numpy as np
import pytest
import torch

import constructed as cs
import near_candidates_ref as R
from parity import assert_state_equal, oracle_for
from test_gpu_parity import obs_check
from test_gpu_rollout import assert_same
from test_gpu_rollout_autoreset import flock_loop, flock_loop_bots, flock_twins
from test_gpu_trajectory import assert_traj, per_step

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.bots import flock_actions as bot_flock  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

BOTH = (R.LIST, R.REBUILD)
ALL = (R.LIST, R.REBUILD, R.PLAIN)


def worlds(E, N, seed, **kw):
    """(per-step twin, rollout with the lists, rollout with MACM_DEBUG_NEAR_PLAIN, oracle)"""
    a, b, c = (FlockVec(E, n_agents=[N], seed=seed, device="cuda:0", **kw) for _ in range(3))
    c.world.set_debug(_abi.DEBUG_NEAR_PLAIN)
    okw = {k: v for k, v in kw.items() if k != "obs_dtype"}
    orc = oracle_for(to_config(flockSettings(**okw), N, 1, obs_f64=True), None, E, seed)
    return a, b, c, orc


def assert_worlds(a, b, c, ctx):
    for v, nm in ((b, "lists"), (c, "plain")):
        assert_same(a, v, f"{ctx} ({nm})")
        pa, ta = a.reward_sums()
        pv, tv = v.reward_sums()
        np.testing.assert_array_equal(pa, pv, err_msg=f"{ctx} ({nm}): reward sums")
        assert ta == tv and v.status() == 0 and a.spilled() == v.spilled(), f"{ctx} ({nm})"


def oracle_positions(orc, C):
    return orc.get_state(C)["pos"].copy()


def run_case(a, b, c, orc, acts, want, ctx, carried=True):
    """One trajectory launch on b and c against K steps of a and of the oracle; the restatement on
    the oracle's positions must show every kind of step in `want`."""
    K = acts.shape[0]
    f64 = b.world.obs.dtype == torch.float64
    ref = per_step(a, acts)
    tb = b.rollout(acts, trajectory=True)
    tc = c.rollout(acts, trajectory=True)
    assert_traj(ref, tb, f"{ctx} (lists)")
    assert_traj(ref, tc, f"{ctx} (plain)")
    assert_worlds(a, b, c, ctx)
    rows = {k: tb[k].cpu().numpy() for k in ("obs", "nbr_id", "reward", "collided", "done")}
    trace = np.zeros((K,) + tuple(b.get_state()["pos"].shape), np.float32)
    for k, act in enumerate(acts.cpu().numpy()):
        r = orc.step(act)
        np.testing.assert_array_equal(rows["nbr_id"][k], r["nbr_id"], err_msg=f"{ctx}: nbr_id, step {k}")
        np.testing.assert_array_equal(rows["reward"][k], r["reward"].astype(np.float32), err_msg=f"{ctx}: reward {k}")
        np.testing.assert_array_equal(rows["collided"][k], r["collided"], err_msg=f"{ctx}: collided {k}")
        obs_check(rows["obs"][k], r["obs"], f64, f"{ctx}: step {k}")
        trace[k] = oracle_positions(orc, b.world.C)
    assert_state_equal(b.get_state(), orc.get_state(b.world.C), f"{ctx}: vs oracle")
    wrong, kinds, largest = R.run_trace(trace, first_step_plain=carried)
    assert wrong == 0
    for kind in want:
        assert (kinds == kind).any(), f"{ctx}: no step of kind {kind} by the restatement"
    return kinds, largest


def cpu_actions(K, E, N, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 3, size=(K, E, N, 3)).astype(np.uint8)).cuda()


# ---- 1. random rollouts: agent counts, observation forms, a dense start -------------------------------
@pytest.mark.parametrize("E,N,K,kw,want", [
    (16, 64, 100, {}, BOTH),
    (64, 64, 64, {}, BOTH),                                   # K >= 32: the balanced launch (wave b steps env order[b])
    (8, 63, 64, {}, BOTH),                                    # lanes >= N in the 64-record kernel
    (8, 33, 64, {}, BOTH),
    (8, 32, 64, {}, ()),                                      # the 32-record kernel: no lists, unaffected
    (8, 64, 64, {"obs_dtype": torch.float64}, BOTH),
    (8, 64, 64, {"coord": "cartesian"}, BOTH),
    (8, 64, 80, {"start_spread": 6}, ALL),                    # dense start: failed rebuilds, plain steps, then lists
], ids=["64", "64-balanced", "63", "33", "32", "f64", "cartesian", "spread6"])
def test_rollout_equals_per_step_plain_and_oracle(E, N, K, kw, want):
    a, b, c, orc = worlds(E, N, 5, **kw)
    kinds, largest = run_case(a, b, c, orc, cpu_actions(K, E, N, 11), want, f"N = {N} {kw}")
    if kw.get("start_spread") == 6:
        assert (largest[kinds == R.REBUILD] > R.CAP).any(), "no list above the cap at the dense start"
    elif want:
        assert ((kinds == R.REBUILD).sum(axis=0) >= 3).all(), "several rebuilds inside the launch, in every env"


def test_spill_steps_inside_the_launch():
    """start_spread 4: some env-steps take the spill step, which clears the lists."""
    E, N, K = 8, 64, 64
    a, b, c, orc = worlds(E, N, 5, start_spread=4)
    s0 = b.spilled()
    run_case(a, b, c, orc, cpu_actions(K, E, N, 11), (R.REBUILD, R.PLAIN), "spread 4")
    assert 0 < b.spilled() - s0 < E * K, b.spilled() - s0


# ---- 2. two launches in a row with a set_state in between ---------------------------------------------
def test_two_launches_with_set_state_between():
    """The lists do not outlive a launch: the second starts from an injected state of another world
    (every position changed behind the kernel's back), and from the first's own end state."""
    E, N, K = 8, 64, 40
    a, b, c, orc = worlds(E, N, 13)
    acts = cpu_actions(3 * K, E, N, 21)
    run_case(a, b, c, orc, acts[:K], BOTH, "first launch")
    d = FlockVec(E, n_agents=[N], seed=99, device="cuda:0")
    for k in range(3):
        d.step(acts[k])
    st = d.get_state()
    for v in (a, b, c):
        v.set_state(st)
    orc.set_state(st)
    run_case(a, b, c, orc, acts[K:2 * K], BOTH, "after set_state")
    run_case(a, b, c, orc, acts[2 * K:], BOTH, "third launch")


# ---- 3. the closed loop: flocks converge, envs go dense and back --------------------------------------
def test_closed_loop_300_steps():
    E, N, K = 8, 64, 300
    a, b, c, orc = worlds(E, N, 12)
    act_a = bot_flock(a.obs)
    acts_b = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device="cuda:0")
    acts_b[0] = act_a
    act_c = act_a.clone()
    rows = {k: [] for k in ("obs", "nbr_id", "reward", "collided", "done")}
    for _ in range(K):
        a.step(act_a)
        for key in rows:
            rows[key].append(getattr(a.world, key).clone())
        bot_flock(a.obs, out=act_a)
    tb = b.rollout_bots(acts_b, K, trajectory=True)
    c.rollout_bots(act_c, K)
    assert_traj({k: torch.stack(v) for k, v in rows.items()}, tb, "closed loop")
    assert torch.equal(acts_b[K], act_a) and torch.equal(act_c, act_a), "the bot's next actions"
    assert_worlds(a, b, c, "closed loop")
    # the oracle through the actions taken, and the restatement on its positions
    trace = np.zeros((K, E, N, 2), np.float32)
    nbr = tb["nbr_id"].cpu().numpy()
    for k, act in enumerate(acts_b[:K].cpu().numpy()):
        r = orc.step(act)
        np.testing.assert_array_equal(nbr[k], r["nbr_id"], err_msg=f"nbr_id, step {k}")
        trace[k] = oracle_positions(orc, b.world.C)
    assert_state_equal(b.get_state(), orc.get_state(b.world.C), "closed loop vs oracle")
    wrong, kinds, largest = R.run_trace(trace)
    assert wrong == 0
    for kind in ALL:
        assert (kinds == kind).any(), kind
    dense = (kinds == R.REBUILD) & (largest > R.CAP)
    first = kinds[:40]
    assert (first == R.LIST).any() and dense[100:].any(), "lists while the flock gathers, dense once it has"


# ---- 4. autoreset: envs end inside the launch ---------------------------------------------------------
@pytest.mark.parametrize("bots", [False, True])
def test_autoreset_inside_the_launch(bots):
    """time_limit 0.25: every env ends at its 16th step, four times inside the launch; the new
    episode's positions have nothing to do with the lists' build positions."""
    E, N, K = 8, 64, 70
    off, on = flock_twins(E, N, 5, time_limit=0.25)
    _, plain = flock_twins(E, N, 5, time_limit=0.25)
    plain.world.set_debug(_abi.DEBUG_NEAR_PLAIN)
    if bots:
        act0 = bot_flock(off.obs)
        ref, arows = flock_loop_bots(off, act0, K)
        for v in (on, plain):
            acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device="cuda:0")
            acts[0] = act0
            assert_traj(ref, v.rollout_bots(acts, K, trajectory=True), "closed loop")
            assert torch.equal(acts, arows)
    else:
        acts = cpu_actions(K, E, N, 11)
        ref = flock_loop(off, acts)
        assert_traj(ref, on.rollout(acts, trajectory=True), "lists")
        assert_traj(ref, plain.rollout(acts, trajectory=True), "plain")
    assert int(ref["done"].sum()) == 4 * E
    assert_same(off, on, "autoreset (lists)")
    assert_same(off, plain, "autoreset (plain)")
    # between two resets an episode of 16 steps has list steps (the restatement on the twin's rows is
    # not available: its positions are not a trajectory output; the default-spread case above is the same start)
    wrong, kinds, _ = R.run_trace(R.oracle_trace(E, N, 16, seed=5, time_limit=0.25)[0], first_step_plain=True)
    assert wrong == 0 and (kinds == R.LIST).any() and (kinds == R.REBUILD).any()


# ---- 5. constructed states ----------------------------------------------------------------------------
def lattice_world(seed, mutate=None, spacing=2.0):
    E, N = 2, 64
    a, b, c, orc = worlds(E, N, seed, start_spread=200)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * spacing
    rng = np.random.default_rng(seed)
    pos = np.stack([g[rng.permutation(N)] for _ in range(E)])  # index order unrelated to the geometry
    v = np.zeros_like(pos)
    if mutate:
        mutate(pos, v)
    cs.inject(a, orc, pos, vel=v)
    st = a.get_state()
    for w in (b, c):
        w.step(torch.ones((E, N, 3), dtype=torch.uint8, device="cuda:0"))  # as inject's idle step
        w.set_state(st)
    return a, b, c, orc, pos


def idle_then_random(K, E, N, hold, seed):
    acts = np.ones((K, E, N, 3), np.uint8)  # (1, 1, 1): no force, no turn
    acts[hold:] = np.random.default_rng(seed).integers(0, 3, size=(K - hold, E, N, 3))
    return torch.from_numpy(acts).cuda()


def test_exact_ties_on_a_lattice():
    """Pitch 2 m, at rest for 10 steps: up to four neighbours at exactly the same d2, the lowest index
    wins, from the lists as from the sweep; then random actions break the ties one by one."""
    a, b, c, orc, pos = lattice_world(3)
    best, _ = R.plain_nearest(pos[0])
    assert ((R.d2_matrix(pos[0]) == best[:, None]).sum(axis=1) >= 2).all()
    kinds, _ = run_case(a, b, c, orc, idle_then_random(64, 2, 64, 10, 4), BOTH, "lattice")
    assert (kinds[2:10] == R.LIST).all(), "the resting lattice takes list steps"


def test_coincident_agents():
    """Two agents at the same point (d2 = 0, atan2(0, 0) in the observation); the solver separates them."""
    def mutate(pos, v):
        pos[:, 40] = pos[:, 7]
    a, b, c, orc, _ = lattice_world(5, mutate)
    run_case(a, b, c, orc, idle_then_random(64, 2, 64, 6, 6), BOTH, "coincident")


def test_fast_agent():
    """An agent at the translation clamp (300 m/s: 2 m per step) flying between two rows of the
    lattice: the displacement test fails at every step of the flight, each of which rebuilds."""
    def mutate(pos, v):
        for e in range(pos.shape[0]):
            i = int(np.argmin(pos[e].sum(axis=1)))  # the corner agent
            pos[e, i] = (-1.0, 1.5)
            v[e, i] = (300.0, 0.0)
    a, b, c, orc, _ = lattice_world(7, mutate, spacing=3.0)
    kinds, _ = run_case(a, b, c, orc, idle_then_random(40, 2, 64, 40, 8), (R.REBUILD,), "fast agent")
    assert (kinds[1:6] == R.REBUILD).all(), "no list step while the agent moves 2 m a step"
