"""The melee ray cast at its boundaries (tests/constructed.raycast_groups), HIP against the CPU
oracle and against tests/raycast_ref.py: kernel, oracle and numpy must agree on every hit.

A cast yields only a hit index, so a different rounding of `a / rr`, `maxFraction * rr` or
`sqrtf(sigma)` shows only where two candidates tie, where the entry point lies at the melee range,
or where the ray is tangent; spawned worlds reach none of these. The scenarios are injected
(constructed.inject_tdm), the attackers take the attack action alone (the cast happens before the
physics), then the reference's combat bot drives two more steps. Forms: the 32-lane wave (teams
[1, 3], one scenario per env), the 64-lane wave ([32, 32]), the workgroup step ([33, 32]) and two
bodies per thread ([513, 512]); each with the reference's shared listener and with fresh_raycast.
The larger forms hold several scenarios per env, so the shared listener carries hits from one
scenario to the next in agent order, as the oracle defines it."""
import numpy as np
import pytest

import constructed as cs
from parity import combat_bot
from test_gpu_tdm import check_rollout, make_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fresh", [0, 1])
@pytest.mark.parametrize("form", list(cs.TDM_FORMS))
def test_raycast_boundaries_match_oracle_and_numpy(form, fresh):
    teams, kw, (pos, ang, alive, health, attack, where) = cs.tdm_form(form)
    E = pos.shape[0]
    w, orc = make_pair(E, teams, seed=3, fresh_raycast=bool(fresh), **kw)
    cs.inject_tdm(w, orc, pos, ang, alive, health)
    want, hits = cs.expected_health(pos, ang, alive, health, attack, fresh)
    assert (hits >= 0).any() and (hits == -1).any()
    t = [0]

    def policy(obs, mask):
        t[0] += 1
        if t[0] == 1:
            return cs.attack_actions(attack)
        if t[0] == 2:  # after the casts: the health that the numpy restatement's hits explain
            np.testing.assert_array_equal(w.health.cpu().numpy(), want)
        return combat_bot(obs, mask)

    attacks = int(w.counters()[1])
    check_rollout(w, orc, 3, policy)
    assert int(w.counters()[1]) - attacks >= int((attack & (alive != 0)).sum())
