"""The Flock step's untaken branches, from constructed states (tests/constructed.py), against the
CPU oracle at the suite's bar (test_gpu_parity.check_rollout: state bitwise, rewards, neighbour
ids and collided exact, observations by obs_check).

A rollout from a random reset never clamps a translation (dt * |v| > 2 m), never has two centres
within b2_epsilon of each other (the manifold's fallback normal (1, 0), Normalize's early return in
the position solver, atan2(0, 0) in the observation), almost never clamps a position correction at
-0.2, and decides `touching` far from its boundary. The scenarios put bodies exactly there, on both
sides of each boundary, in every form of the step: the 32-lane wave (N = 4, one group per env), the
64-lane wave, the forced spill step, the workgroup step (N = 65) and two bodies per thread
(N = 1025). tests/test_oracle_constructed.py shows without a GPU that the oracle takes each
branch."""
import numpy as np
import pytest
import torch

import constructed as cs
from parity import assert_state_equal
from test_gpu_parity import check_rollout, make_pair, obs_check

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402

FORMS = {  # N, one group per env, envs, debug flags, most steps
    "wave32": (4, True, None, 0, 9),
    "wave64": (64, False, 2, 0, 9),
    "forced_spill": (64, False, 2, _abi.DEBUG_FORCE_SPILL, 9),
    "workgroup": (65, False, 2, 0, 9),
    "two_per_thread": (1025, False, 1, 0, 3),
}


def constructed_pair(sc, form, seed=1, groups=None):
    N, one_per_env, E, debug, _ = FORMS[form]
    pos, vel, ang, act, where = cs.flock_layout(groups or sc["groups"], N, one_per_env, spacing=sc["spacing"],
                                                radius=sc["radius"], E=E or 2)
    vec, orc = make_pair(pos.shape[0], [N], seed, start_spread=200, **sc["kw"])
    if debug:
        vec.world.set_debug(debug)
    cs.inject(vec, orc, pos, vel=vel, angle=ang, radius=sc["radius"])
    return vec, orc, act


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", cs.FLOCK_SCENARIOS)
def test_constructed_scenario_matches_oracle(name, form):
    sc = cs.flock_scenario(name)
    vec, orc, act = constructed_pair(sc, form)
    rng = np.random.default_rng(7)
    steps = min(sc["hold"] + sc["random"], FORMS[form][4])
    spilled = vec.spilled()
    check_rollout(vec, orc, steps, rng, actions_fn=cs.scenario_actions(sc, act, rng))
    if form == "forced_spill":
        assert vec.spilled() - spilled == steps * vec.num_envs


def test_carried_rollout_from_constructed_state():
    """Scenarios a and c in one 64-agent world through FlockVec.rollout (K = 4: the wave keeps the
    env's state in registers between the steps): final state and last outputs equal the oracle's."""
    sc = cs.flock_scenario("fast")
    groups = cs.sub_eps_pairs() + cs.fast_bodies()
    vec, orc, act = constructed_pair(sc, "wave64", seed=2, groups=groups)
    rng = np.random.default_rng(11)
    fn = cs.scenario_actions(dict(hold=2), act, rng)
    acts = np.stack([fn(t) for t in range(4)])
    obs, nbr = vec.rollout(torch.from_numpy(acts).cuda())[:2]
    for t in range(4):
        r = orc.step(acts[t])
    w = vec.world
    np.testing.assert_array_equal(w.reward.cpu().numpy(), r["reward"].astype(np.float32))
    np.testing.assert_array_equal(w.nbr_id.cpu().numpy(), r["nbr_id"])
    np.testing.assert_array_equal(w.collided.cpu().numpy(), r["collided"])
    np.testing.assert_array_equal(w.done.cpu().numpy(), r["done"])
    obs_check(w.obs.cpu().numpy(), r["obs"], False, "rollout")
    assert_state_equal(vec.get_state(), orc.get_state(w.C), "after the rollout")
    assert vec.status() == 0
