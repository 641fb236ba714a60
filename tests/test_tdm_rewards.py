"""gym_macm.tdm_rewards on CPU tensors against a plain Python loop, over the events derived from
the oracle (tdm_events_ref) and the oracle's own outputs of fixtures W1 (literal listener), W2
(fresh_raycast) and W6 (episodes that end and restart). The weights are dyadic, so every partial sum
of the float32 terms is exact and the comparison is equality."""
import numpy as np
import pytest
import torch
from tdm_events_ref import FIXTURES, fixture_config, run_fixture

from gym_macm import tdm_rewards

DEFAULTS = dict(hit_enemy=1.0, hit_ally=-1.0, hurt=-1.0, death=-1.0, win=4.0, loss=-4.0)
OTHER = dict(hit_enemy=0.5, hit_ally=-2.0, hurt=-0.25, death=-8.0, win=16.0, loss=-0.125)


def team_of(name):
    return np.repeat(np.arange(len(FIXTURES[name][0])), FIXTURES[name][0]).astype(np.int32)


def loop_events(hit, team, alive_before):
    K, E, N = hit.shape
    he, ha, hu = (np.zeros((K, E, N), np.int32) for _ in range(3))
    hu_all = np.zeros((K, E, N), np.int32)
    for k in range(K):
        for e in range(E):
            for i in range(N):
                v = hit[k, e, i]
                if v < 0:
                    continue
                hu_all[k, e, v] += 1
                if alive_before[k, e, v]:
                    hu[k, e, v] += 1
                if alive_before[k, e, i]:
                    if team[v] != team[i]:
                        he[k, e, i] = 1
                    else:
                        ha[k, e, i] = 1
    return he, ha, hu, hu_all


def loop_rewards(t, team, w, he, ha, hu):
    K, E, N = t["hit_id"].shape
    r = np.zeros((K, E, N), np.float32)
    f = np.float32
    for k in range(K):
        for e in range(E):
            first = bool(t["done"][k, e]) and not bool(t["done_before"][k, e]) and t["winner"][k, e] >= 0
            for i in range(N):
                died = bool(t["alive_before"][k, e, i]) and not bool(t["alive"][k, e, i])
                won = first and team[i] == t["winner"][k, e]
                lost = first and team[i] != t["winner"][k, e]
                x = f(w["hit_enemy"]) * f(he[k, e, i])
                x = f(x + f(w["hit_ally"]) * f(ha[k, e, i]))
                x = f(x + f(w["hurt"]) * f(hu[k, e, i]))
                x = f(x + f(w["death"]) * f(died))
                x = f(x + f(w["win"]) * f(won))
                x = f(x + f(w["loss"]) * f(lost))
                r[k, e, i] = x
    return r


@pytest.mark.parametrize("name", ["W1", "W2", "W6"])
def test_events_and_rewards_match_the_loop(name):
    t, team = run_fixture(name), team_of(name)
    he, ha, hu, hu_all = loop_events(t["hit_id"], team, t["alive_before"])
    T = {k: torch.from_numpy(np.array(t[k])) for k in ("hit_id", "alive_before", "alive", "done", "done_before", "winner")}
    ge, ga, gu = tdm_rewards.combat_events(T["hit_id"], torch.from_numpy(team), T["alive_before"])
    for got, want, what in ((ge, he, "hit_enemy"), (ga, ha, "hit_ally"), (gu, hu, "hurt")):
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        np.testing.assert_array_equal(got.numpy(), want, err_msg=f"{name}: {what}")
    # one step's [E, N] rows give the trajectory's row
    g0 = tdm_rewards.combat_events(T["hit_id"][3], team, T["alive_before"][3])
    np.testing.assert_array_equal(g0[2].numpy(), hu[3])
    for w in (DEFAULTS, OTHER):
        got = tdm_rewards.combat_rewards(T["hit_id"], T["alive_before"], T["alive"], T["done"], T["done_before"],
                                         T["winner"], team, **({} if w is DEFAULTS else w))
        assert got.dtype == torch.float32
        np.testing.assert_array_equal(got.numpy(), loop_rewards(t, team, w, he, ha, hu), err_msg=f"{name}: rewards")
    # every unit of damage is an event: health falls by melee_dmg per attacker, the mask aside
    dmg = float(fixture_config(name).melee_dmg)
    np.testing.assert_array_equal(t["health_before"] - t["health"], hu_all * dmg)
    assert int(he.sum()) > 0 and int(hu.sum()) > 0
    if name == "W1":
        assert int(ha.sum()) > 0 and int((hu_all - hu).sum()) > 0  # allies hit, and damage on the dead


def test_w6_has_wins_or_time_limits_only_once_per_episode():
    t, team = run_fixture("W6"), team_of("W6")
    T = {k: torch.from_numpy(np.array(t[k])) for k in ("hit_id", "alive_before", "alive", "done", "done_before", "winner")}
    zero = dict(hit_enemy=0.0, hit_ally=0.0, hurt=0.0, death=0.0)
    r = tdm_rewards.combat_rewards(T["hit_id"], T["alive_before"], T["alive"], T["done"], T["done_before"], T["winner"],
                                   team, win=4.0, loss=-4.0, **zero).numpy()
    ended = (t["done"] != 0) & (t["done_before"] == 0) & (t["winner"] >= 0)
    assert ((r != 0).any(axis=-1) == ended).all()
    for k, e in np.argwhere(ended):
        np.testing.assert_array_equal(r[k, e], np.where(team == t["winner"][k, e], 4.0, -4.0).astype(np.float32))


@pytest.mark.parametrize("name,autoreset", [("W1", False), ("W6", True)])
def test_trajectory_alive_before(name, autoreset):
    t = run_fixture(name)
    alive0 = torch.ones(t["alive"].shape[1:], dtype=torch.uint8)
    got = tdm_rewards.trajectory_alive_before(alive0, torch.from_numpy(np.array(t["alive"])),
                                              torch.from_numpy(np.array(t["done"])), autoreset=autoreset)
    np.testing.assert_array_equal(got.numpy(), t["alive_before"])
    if autoreset:  # without the flag the rows after an end are the terminal step's, not the respawn's
        plain = tdm_rewards.trajectory_alive_before(alive0, torch.from_numpy(np.array(t["alive"])),
                                                    torch.from_numpy(np.array(t["done"])))
        assert not np.array_equal(plain.numpy(), t["alive_before"])
