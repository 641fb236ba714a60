"""tdm_events_ref.derive_events is the oracle's melee: on every fixture the events tests use, for
every step, the replayed health and listener equal the oracle's post-step health and
extras()['listener'] bit for bit; and the fixtures hold the cases they were chosen for (the minimum
counts are about half of what the fixtures give, so that a changed generator is noticed, not a
changed draw)."""
import numpy as np
import pytest
from tdm_events_ref import FIXTURES, event_counts, fixture_config, run_fixture


@pytest.mark.parametrize("name", list(FIXTURES))
def test_replay_is_the_oracles(name):
    t = run_fixture(name)
    K = t["hit_id"].shape[0]
    for k in range(K):
        np.testing.assert_array_equal(t["health_ref"][k], t["health"][k], err_msg=f"{name}: health after step {k}")
        np.testing.assert_array_equal(t["listener_ref"][k], t["listener"][k], err_msg=f"{name}: listener after step {k}")
    hit = t["hit_id"]
    N = hit.shape[-1]
    assert hit.dtype == np.int32 and hit.min() >= -1 and hit.max() < N
    # an entry only where an attack could be made, and with fresh_raycast only the ray's own body
    att = (t["alive_before"] != 0) & (t["cd_atk_before"] <= 0.0) & (t["actions"][..., 3] != 0)
    assert not ((hit >= 0) & ~att).any()
    if fixture_config(name).fresh_raycast:
        np.testing.assert_array_equal(hit, t["ray_hit"])


MINIMA = {
    "W1": dict(damaging=500, stale=500, self=5, dead=500),
    "W2": dict(damaging=50),
    "W3": dict(damaging=20),
    "G1": dict(damaging=100),
    "G1f": dict(damaging=40),
    "G2": dict(damaging=100),
    "G3": dict(damaging=100),
}


@pytest.mark.parametrize("name", list(MINIMA))
def test_fixture_holds_its_cases(name):
    c = event_counts(fixture_config(name), run_fixture(name))
    for k, least in MINIMA[name].items():
        assert c[k] >= least, (name, k, c)
    if name == "W2":
        assert c["stale"] == 0, c  # a fresh listener damages only what the ray hit


def test_w6_ends_and_goes_on():
    """Every env ends at least twice, and damage is dealt in the episodes after an end."""
    t = run_fixture("W6")
    done = t["done"] != 0
    assert (done.sum(axis=0) >= 2).all(), done.sum(axis=0)
    after = np.cumsum(done, axis=0) - done > 0  # steps after an env's first end
    assert int(((t["hit_id"] >= 0) & after[..., None]).sum()) >= 100
    # the first attack after a reset sees a fresh listener: nothing is damaged before a ray hits
    k_e = np.argwhere(done[:-1])
    fresh = 0
    for k, e in k_e:
        assert (t["listener_before"][k + 1, e] == (0, -1)).all()
        fresh += 1
    assert fresh >= 32
