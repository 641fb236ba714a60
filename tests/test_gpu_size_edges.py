"""Agent counts at the dispatch edges, against the CPU oracle (state bit for bit, observations as
test_gpu_parity / test_gpu_tdm check them). The code changes form at N <= 32 (the 32-lane wave
instantiation, TDM's 6 KB observation stage), N <= 64 (wave or workgroup), multiples of 64 (wg_block),
N <= 1024 (one body per thread), N <= 2048 (two, above that four). The counts just inside and just
outside each edge that no other test runs: the minimum N = 2 (TDM's default [1, 1]), 3, 31, 63, 1025
(exactly one thread holds a second body), 2049 and 3073 (one thread holds a third / fourth body, most
slots of the last pass empty), TDM 63 and 64 beside the existing 65, and TDM 1025."""
import numpy as np
import pytest
import torch

from parity import combat_bot
from test_gpu_parity import check_rollout, make_pair
from test_gpu_tdm import check_rollout as tdm_check_rollout
from test_gpu_tdm import make_pair as tdm_make_pair

pytestmark = pytest.mark.gpu

from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402


@pytest.mark.parametrize("obs_dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [2, 3, 31, 32, 63])
def test_flock_wave_edge_counts(N, obs_dtype):
    """The wave kernel at N = 2 (the minimum: one pair, lane 0's neighbour is lane 1 and the reverse),
    3, 31 / 32 (the last counts of the 32-lane instantiation) and 63 (one idle lane of the 64-lane one),
    crowded enough that agents collide (the solver, islands and contact list run, not only free flight)."""
    vec, orc = make_pair(4, [N], seed=N, start_spread=max(2, N / 6), obs_dtype=obs_dtype)
    check_rollout(vec, orc, 40, np.random.default_rng(N), state_every=10, obs_f64=obs_dtype == torch.float64)
    assert vec.counters()[1] > 0, "no agent collided: the contact path never ran"


@pytest.mark.parametrize("N", [2, 63])
def test_flock_wave_edge_counts_continuous_cartesian(N):
    """The same edges through the continuous action decode (float2 per agent) and the 6-wide cartesian
    observation row (scalar stores, not the polar row's one vector)."""
    E = 4
    vec, orc = make_pair(E, [N], seed=N, start_spread=max(2, N / 6), action_mode="continuous", coord="cartesian")
    rng = np.random.default_rng(N)
    check_rollout(vec, orc, 40, None, state_every=10,
                  actions_fn=lambda t: rng.uniform(-1, 1, size=(E, N, 2)).astype(np.float32))
    assert vec.counters()[1] > 0, "no agent collided: the contact path never ran"


@pytest.mark.parametrize("N,spread,steps", [(1025, 30.0, 4), (2049, 60.0, 4), (3073, 80.0, 3)])
def test_flock_big_edge_counts(N, spread, steps):
    """The big path (N > 1024: the spill step with 2 or 4 bodies per thread) where exactly one thread
    holds a body in the last slot: N = 1025 (2 per thread), 2049 and 3073 (4 per thread, the third / fourth
    slot of one thread). Then reset_envs and two more steps: the big init kernel's chunk loop with a
    partial last chunk of one body."""
    vec, orc = make_pair(1, [N], seed=N, start_spread=spread)
    check_rollout(vec, orc, steps, np.random.default_rng(N), state_every=2)
    assert vec.spilled() == steps, "N > 1024 steps every env with the spill step"
    assert vec.counters()[1] > 0
    vec.reset_envs()
    orc.reset_envs()
    check_rollout(vec, orc, 2, np.random.default_rng(N + 1), state_every=1)  # starts with state and obs at reset
    assert vec.spilled() == steps + 2


@pytest.mark.parametrize("teams", [[1, 1], [2, 1]])
def test_tdm_minimum_teams_to_the_end(teams):
    """TDM at its minimum and default size [1, 1] (N = 2: one observation slot per agent, one pair) and
    [2, 1], in a 6 x 6 world until every episode has ended. [1, 1]: envs where both agents die in the
    same step (done with winner -1, the alive_teams == 0 branch) beside one with a winner; [2, 1]: a
    winner in every env."""
    E = 4
    w, orc = tdm_make_pair(E, teams, seed=3, world_width=6.0, world_height=6.0)
    r = tdm_check_rollout(w, orc, 400, combat_bot, state_every=20)
    done, winner = w.done.cpu().numpy(), w.winner.cpu().numpy()
    assert (done == 1).all(), done
    if teams == [1, 1]:
        assert ((done == 1) & (winner == -1)).any(), "no env ended with both agents dead in one step"
        assert (winner >= 0).any(), "no env ended with a winner"
    else:
        assert (winner >= 0).all(), winner
    assert int(w.counters()[1]) > 0 and (r["alive"] == 0).any()


@pytest.mark.parametrize("teams", [[32, 31], [32, 32]])
def test_tdm_wave_edge_counts(teams):
    """TDM at N = 63 and 64, the wave kernel's last counts (the workgroup step starts at the tested 65):
    120 bot steps in a crowded world with melee attacks, then a trajectory rollout of 5 steps from that
    state equals per-step stepping (the rollout kernel's 64-lane instantiation, its observation rows)."""
    E, N, K = 4, sum(teams), 5
    kw = dict(world_width=14.0, world_height=14.0)
    w, orc = tdm_make_pair(E, teams, seed=N, **kw)
    tdm_check_rollout(w, orc, 120, combat_bot, state_every=20)
    assert int(w.counters()[1]) > 0, "no melee attack"
    b = TdmWorld(tdm_config(teams, **kw), E, device="cuda:0")
    b.reset(N, 0)
    b.set_state(w.get_state())
    g = torch.Generator(device="cuda:0")
    g.manual_seed(N)
    acts = torch.randint(0, 3, (K, E, N, 4), dtype=torch.uint8, device="cuda:0", generator=g)
    acts[..., 3] = torch.randint(0, 2, (K, E, N), dtype=torch.uint8, device="cuda:0", generator=g)
    keys = TdmWorld._TRAJ_KEYS
    ref = {k: [] for k in keys}
    for k in range(K):
        w.step(acts[k])
        for key, t in zip(keys, w.outputs()):
            ref[key].append(t.clone())
    traj = b.rollout_traj(acts)
    for key in keys:
        assert torch.equal(torch.stack(ref[key]), traj[key]), f"trajectory rollout: {key}"
    sa, sb = w.get_state(), b.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"state[{k}]")
    assert w.status() == 0 and b.status() == 0


def test_tdm_two_bodies_per_thread_edge():
    """TDM [513, 512] (N = 1025): the workgroup step with two bodies per thread, one thread holding the
    only body of the second pass."""
    w, orc = tdm_make_pair(1, [513, 512], seed=1025, world_width=60.0, world_height=60.0)
    tdm_check_rollout(w, orc, 6, combat_bot, state_every=2)
    assert w.spilled() == 6, "every env-step above 64 agents is the workgroup step's"
