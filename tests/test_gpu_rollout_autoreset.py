"""Autoreset inside rollouts (macm_world_set_autoreset / macm_tdm_set_autoreset): an env whose step k
sets done restarts before step k + 1, on the wave path inside the rollout launch (env_rollout_ar_w64,
csrc/rollout_autoreset.inc), on the workgroup path by the draw and init launches after each step's.

The bar: a twin world with the same seed and autoreset off, driven by the per-step loop
`step -> copy the terminal fields -> reset_envs(copy of done) -> read obs / nbr_id / mask [-> bots]`,
gives every trajectory row, the final get_state, the counters and the reward sums bit for bit; the
final states also equal the oracle's (orc.step + orc.reset_envs). Row k keeps the terminal done,
reward, collided (TDM: winner, health, alive) and holds the new episode's initial obs for reset envs."""
import ctypes

import numpy as np
import pytest
import torch

from guard_bands import GuardedOutputs
from oracle import OracleTDM
from parity import assert_state_equal, oracle_for
from test_gpu_rollout import assert_same, flock_actions
from test_gpu_tdm import assert_tdm_state_equal
from test_gpu_trajectory import assert_tdm_state, assert_traj

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.bots import flock_actions as bot_flock  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

FKEYS = ("obs", "nbr_id", "reward", "collided", "done")
TKEYS = TdmWorld._TRAJ_KEYS
MT_WORDS = 624  # MT19937 state words: a draw past them twists


# ---- the per-step loop of a world with autoreset off (the parent commit's only form) ----------------
def flock_loop_step(vec, act):
    """One iteration: row k of a trajectory with autoreset on."""
    w = vec.world
    w.step(act)
    row = {k: getattr(w, k).clone() for k in ("reward", "collided", "done")}  # the terminal fields
    w.reset_envs(row["done"].clone())  # a copy: the world's own done output keeps its 1
    row["obs"], row["nbr_id"] = w.obs.clone(), w.nbr_id.clone()
    return row


def flock_loop(vec, acts):
    rows = [flock_loop_step(vec, acts[k]) for k in range(acts.shape[0])]
    return {k: torch.stack([r[k] for r in rows]) for k in FKEYS}


def flock_loop_bots(vec, act, K):
    """The closed loop; returns the trajectory and the K + 1 action rows."""
    act = act.clone()
    rows, arows = [], [act.clone()]
    for _ in range(K):
        rows.append(flock_loop_step(vec, act))
        bot_flock(vec.world.obs, out=act)  # a reset env: from its new initial obs
        arows.append(act.clone())
    return {k: torch.stack([r[k] for r in rows]) for k in FKEYS}, torch.stack(arows)


def tdm_loop_step(w, act):
    w.step(act)
    row = {k: getattr(w, k).clone() for k in ("health", "alive", "done", "winner")}  # terminal
    w.reset_envs(row["done"].clone())  # overwrites the world's health / alive / winner outputs too
    row["obs"], row["mask"] = w.obs.clone(), w.mask.clone()
    return row


def tdm_loop(w, acts):
    rows = [tdm_loop_step(w, acts[k]) for k in range(acts.shape[0])]
    return {k: torch.stack([r[k] for r in rows]) for k in TKEYS}


def tdm_loop_bots(w, act, K):
    act = act.clone()
    rows, arows = [], [act.clone()]
    for _ in range(K):
        rows.append(tdm_loop_step(w, act))
        combat_actions(w.obs, w.mask, out=act)
        arows.append(act.clone())
    return {k: torch.stack([r[k] for r in rows]) for k in TKEYS}, torch.stack(arows)


def flock_twins(E, N, seed, **kw):
    """(autoreset off, autoreset on), the same seed"""
    off = FlockVec(E, n_agents=[N], seed=seed, device="cuda:0", **kw)
    on = FlockVec(E, n_agents=[N], seed=seed, device="cuda:0", autoreset=True, **kw)
    return off, on


def assert_flock_end(off, on, ctx, outputs=True):
    """State, counters (and the worlds' current outputs), reward sums, spilled, status."""
    if outputs:
        assert_same(off, on, ctx)
    else:
        sa, sb = off.get_state(), on.get_state()
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{ctx}: state[{k}]")
        np.testing.assert_array_equal(off.counters(), on.counters(), err_msg=f"{ctx}: counters")
    pa, ta = off.reward_sums()
    pb, tb = on.reward_sums()
    np.testing.assert_array_equal(pa, pb, err_msg=f"{ctx}: reward sums")
    assert ta == tb, f"{ctx}: reward total"
    assert off.spilled() == on.spilled(), f"{ctx}: spilled"
    assert off.status() == 0 and on.status() == 0


def flock_oracle_replay(E, N, seed, segments, **kw):
    """The oracle through the same calls: segments of ("step", acts [K, E, N, A]) with a reset on
    every step's done flags, or ("reset", mask)."""
    okw = {k: v for k, v in kw.items() if k != "obs_dtype"}
    orc = oracle_for(to_config(flockSettings(**okw), N, 1, obs_f64=True), None, E, seed)
    dones = 0
    for what, x in segments:
        if what == "reset":
            orc.reset_envs(x)
            continue
        for a in x.cpu().numpy():
            r = orc.step(a)
            if r["done"].any():
                orc.reset_envs(r["done"])
                dones += int(r["done"].sum())
    return orc, dones


def tdm_twins(teams, E, seed, obs_f64=False, **cfg):
    off = TdmWorld(tdm_config(teams, obs_f64=obs_f64, **cfg), E, device="cuda:0")
    on = TdmWorld(tdm_config(teams, obs_f64=obs_f64, **cfg), E, device="cuda:0", autoreset=True)
    off.reset(seed)
    on.reset(seed)
    return off, on


def tdm_random_actions(K, E, N, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    acts = torch.randint(0, 3, (K, E, N, 4), dtype=torch.uint8, device="cuda:0", generator=g)
    acts[..., 3] = torch.randint(0, 2, (K, E, N), dtype=torch.uint8, device="cuda:0", generator=g)
    return acts


# ---- 1. Flock N = 64: two groups of envs that end at different steps, a twist on the first reset ----
@pytest.mark.parametrize("reload", [0, 1])
@pytest.mark.parametrize("kw", [{}, {"obs_dtype": torch.float64, "coord": "cartesian"}], ids=["f32polar", "f64cart"])
def test_flock_64_two_phases_in_one_launch(kw, reload):
    E, N, K, seed = 8, 64, 40, 5
    # 2 random() per target and 3 per agent, two words each: construction leaves the stream at 388
    # of its 624 words, so the first reset of 384 words already crosses a twist
    assert 4 + 6 * N < MT_WORDS < 4 + 2 * 6 * N
    off, on = flock_twins(E, N, seed, time_limit=0.25, **kw)
    if reload:
        on.world.set_debug(_abi.DEBUG_ROLLOUT_RELOAD)
    pre = flock_actions(5, E, N, 3)
    for k in range(5):
        off.step(pre[k])
        on.step(pre[k])
    half = torch.tensor([e % 2 for e in range(E)], dtype=torch.uint8, device="cuda:0")
    off.reset_envs(half)
    on.reset_envs(half)
    acts = flock_actions(K, E, N, 11)
    ref = flock_loop(off, acts)
    traj = on.rollout(acts, trajectory=True)
    assert_traj(ref, traj, "trajectory")
    done = traj["done"].cpu().numpy()
    # done at an env's 16th step: the envs not reset above end at rows 10 and 26, the others at 15 and 31
    assert [list(np.flatnonzero(done[:, e])) for e in (0, 1)] == [[10, 26], [15, 31]]
    assert_flock_end(off, on, "after the rollout")
    orc, dones = flock_oracle_replay(E, N, seed, [("step", pre), ("reset", half.cpu().numpy()), ("step", acts)],
                                     time_limit=0.25, **kw)
    assert dones == 2 * E
    assert_state_equal(on.get_state(), orc.get_state(on.world.C), "vs oracle")


# ---- 2. the NCAP = 32 instantiation (three resets to cross a twist), N = 3, continuous actions -----
@pytest.mark.parametrize("N,K,kw", [
    (32, 56, {}),
    (32, 56, {"obs_dtype": torch.float64}),
    (3, 40, {}),
    (32, 40, {"action_mode": "continuous"}),
    (64, 20, {"action_mode": "continuous"}),
])
def test_flock_instantiations(N, K, kw):
    E, seed = 4, 9
    if N == 32 and K == 56:  # 196 words at construction, then 388, 580 and, past 624, the third reset at step 48
        assert 4 + 3 * 6 * N < MT_WORDS < 4 + 4 * 6 * N and K > 48
    off, on = flock_twins(E, N, seed, time_limit=0.25, **kw)
    acts = flock_actions(K, E, N, 21, kw.get("action_mode") == "continuous")
    assert_traj(flock_loop(off, acts), on.rollout(acts, trajectory=True), f"N = {N} {kw}")
    assert_flock_end(off, on, f"N = {N} {kw}")
    orc, dones = flock_oracle_replay(E, N, seed, [("step", acts)], time_limit=0.25, **kw)
    assert dones == E * (K // 16)
    assert_state_equal(on.get_state(), orc.get_state(on.world.C), "vs oracle")


# ---- 3. launch edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(15, 1, 24), (16, 16)], ids=["15+1+24", "16+16"])
def test_flock_launch_edges(lengths):
    """15, 1, 24: a reset in a launch's last (and only) step, then a launch whose first step follows
    a reset. 16 twice: the reset in the last step at both list parities."""
    E, N = 8, 64
    off, on = flock_twins(E, N, 13, time_limit=0.25)
    for i, K in enumerate(lengths):
        acts = flock_actions(K, E, N, 30 + i)
        ref = flock_loop(off, acts)
        traj = on.rollout(acts, trajectory=True)
        assert_traj(ref, traj, f"launch {i} of {K}")
        assert_flock_end(off, on, f"after launch {i} of {K}")
    assert int(on.counters()[3]) == E * (sum(lengths) // 16)


# ---- 4. overwrite form: the last step is an episode end ----------------------------------------------
@pytest.mark.parametrize("N", [64, 20])
def test_flock_overwrite_form_ends_on_done(N):
    E, K = 8, 16
    off, on = flock_twins(E, N, 17, time_limit=0.25)
    acts = flock_actions(K, E, N, 41)
    ref = flock_loop(off, acts)
    obs, nbr, rew, done = on.rollout(acts)
    assert bool(done.all()), "every env ends in the last step"
    for k, t in zip(("obs", "nbr_id", "reward", "done"), (obs, nbr, rew, done)):
        assert torch.equal(t, ref[k][K - 1]), k
    assert torch.equal(on.world.collided, ref["collided"][K - 1])
    assert_flock_end(off, on, "overwrite form")
    assert int(on.get_state()["step_count"].max()) == 0  # the new episodes have not stepped


# ---- 5. Flock closed loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("trajectory", [False, True])
def test_flock_closed_loop(trajectory):
    E, N, K = 8, 64, 40
    off, on = flock_twins(E, N, 19, time_limit=0.25, obs_dtype=torch.float64, coord="cartesian")
    act0 = bot_flock(off.obs)
    ref, arows = flock_loop_bots(off, act0, K)
    if trajectory:
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device="cuda:0")
        acts[0] = act0
        traj = on.rollout_bots(acts, K, trajectory=True)
        assert_traj(ref, traj, "closed-loop trajectory")
        assert torch.equal(acts, arows), "the action rows (after a reset: from the new initial obs)"
        # the rows after the resets at steps 16 and 32 are the bot's on the initial obs in the trajectory
        for k in (15, 31):
            assert bool(traj["done"][k].all())
            assert torch.equal(acts[k + 1], bot_flock(traj["obs"][k]))
    else:
        act = act0.clone()
        on.rollout_bots(act, K)
        assert torch.equal(act, arows[K]), "the bot's next actions"
    assert_flock_end(off, on, "closed loop")


# ---- 6. TDM: episodes that combat ends, at a different step in every env -----------------------------
def test_tdm_combat_ended_episodes():
    E, teams, seed, K, launches = 16, [4, 4], 31, 200, 3
    cfg = dict(world_width=8.0, world_height=8.0)
    off, on = tdm_twins(teams, E, seed, **cfg)
    assert on.launch_flags() == 0
    orc = OracleTDM(tdm_config(teams, obs_f64=True, **cfg), E, seed)
    act = combat_actions(off.obs, off.mask)
    acts = torch.empty((K + 1, E, 8, 4), dtype=torch.uint8, device="cuda:0")
    buf = on.trajectory_buffers(K)
    ends = []
    for i in range(launches):
        ref, arows = tdm_loop_bots(off, act, K)
        acts[0] = act
        traj = on.rollout_bots_traj(acts, K, buf)
        assert_traj(ref, traj, f"launch {i}")
        assert torch.equal(acts, arows), f"launch {i}: action rows"
        act = arows[K].clone()
        done = traj["done"].cpu().numpy().astype(bool)
        winner, alive = traj["winner"].cpu().numpy(), traj["alive"].cpu().numpy()
        health = traj["health"].cpu().numpy()
        for k, e in zip(*np.nonzero(done)):
            ends.append(i * K + k)
            # the terminal values, not the new episode's: at most one team stands (or the time ran out)
            teams_alive = {int(t) for t in on.team[alive[k, e] != 0]}
            assert len(teams_alive) <= 1 and (winner[k, e] == -1) == (len(teams_alive) == 0)
            assert not (alive[k, e] != 0).all() and (health[k, e][alive[k, e] == 0] <= 0).all()
        for a in acts[:K].cpu().numpy():  # the oracle through the actions taken
            r = orc.step(a)
            if r["done"].any():
                orc.reset_envs(r["done"])
    assert len(ends) > E and len(set(ends)) > 1, "episodes ended, at different steps"
    assert_tdm_state(off, on)
    assert_tdm_state_equal(on.get_state(), orc.get_state(), "vs oracle")
    assert on.status() == 0 and off.spilled() == on.spilled()


# ---- 7. TDM instantiations, time-limit ends ----------------------------------------------------------
@pytest.mark.parametrize("teams,bots,obs_f64", [([32, 32], False, False), ([32, 32], True, False),
                                                ([32, 32], False, True), ([16, 16], False, False),
                                                ([16, 16], True, True)])
def test_tdm_time_limit_ends(teams, bots, obs_f64):
    E, K, N = 4, 20, sum(teams)
    if N == 64:  # 384 words at construction and 384 per reset: the first reset crosses a twist
        assert 6 * N < MT_WORDS < 2 * 6 * N
    off, on = tdm_twins(teams, E, 7, obs_f64=obs_f64, time_limit=0.25)
    assert on.launch_flags() == 0
    on.reserve(K)  # valid, a no-op
    if bots:
        act0 = combat_actions(off.obs, off.mask)
        ref, arows = tdm_loop_bots(off, act0, K)
        acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device="cuda:0")
        acts[0] = act0
        traj = on.rollout_bots_traj(acts, K)
        assert torch.equal(acts, arows)
    else:
        acts = tdm_random_actions(K, E, N, 5)
        ref = tdm_loop(off, acts)
        traj = on.rollout_traj(acts)
    assert_traj(ref, traj, f"TDM {teams}")
    assert bool(traj["done"][15].all()) and int(traj["done"].sum()) == E
    assert bool((traj["winner"][15] == -1).all())
    assert_tdm_state(off, on)
    # the overwrite form from here: 16 more steps end on the next time limit
    if not bots:
        acts2 = tdm_random_actions(16, E, N, 6)
        ref2 = tdm_loop(off, acts2)
        on.rollout(acts2)
        for k, t in zip(TKEYS, on.outputs()):
            assert torch.equal(t, ref2[k][15]), f"overwrite form: {k}"
        assert_tdm_state(off, on)


# ---- 8. workgroup path -------------------------------------------------------------------------------
@pytest.mark.parametrize("bots", [False, True])
def test_flock_workgroup_path(bots):
    E, N, K = 4, 100, 20
    off, on = flock_twins(E, N, 23, time_limit=0.25, start_spread=12)
    assert on.world.rollout_slices() == 0
    if bots:
        act0 = bot_flock(off.obs)
        ref, arows = flock_loop_bots(off, act0, K)
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device="cuda:0")
        acts[0] = act0
        traj = on.rollout_bots(acts, K, trajectory=True)
        assert torch.equal(acts, arows)
    else:
        acts = flock_actions(K, E, N, 51)
        ref = flock_loop(off, acts)
        traj = on.rollout(acts, trajectory=True)
    assert_traj(ref, traj, "workgroup path")
    assert bool(traj["done"][15].all())
    assert_flock_end(off, on, "workgroup path")


@pytest.mark.parametrize("bots", [False, True])
def test_tdm_workgroup_path(bots):
    E, teams, K, N = 4, [40, 40], 20, 80
    off, on = tdm_twins(teams, E, 11, time_limit=0.25)
    if bots:
        act0 = combat_actions(off.obs, off.mask)
        ref, arows = tdm_loop_bots(off, act0, K)
        acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device="cuda:0")
        acts[0] = act0
        traj = on.rollout_bots_traj(acts, K)
        assert torch.equal(acts, arows)
    else:
        acts = tdm_random_actions(K, E, N, 8)
        ref = tdm_loop(off, acts)
        traj = on.rollout_traj(acts)
    assert_traj(ref, traj, "TDM workgroup path")
    assert bool(traj["done"][15].all())
    assert_tdm_state(off, on)


# ---- 9. guard bands: the reset writes nothing outside the set fields' extents ------------------------
def test_flock_guard_bands_obs_null():
    E, N, K = 8, 64, 20
    off, on = flock_twins(E, N, 29, time_limit=0.25)
    acts = flock_actions(K, E, N, 61)
    ref = flock_loop(off, acts)
    go = GuardedOutputs(on.world, ("nbr_id", "reward", "collided", "done"), n_steps=K)
    w = on.world
    _abi.check(w.L.macm_world_rollout_traj(w.h, ctypes.c_void_p(acts.data_ptr()), K, go.ref(), w._stream()),
               "macm_world_rollout_traj")
    go.assert_equal(ref, "Flock, obs NULL")
    assert bool(go["done"][15].all())
    assert_flock_end(off, on, "guarded", outputs=False)


def test_tdm_guard_bands():
    E, teams, K, N = 4, [16, 16], 20, 32
    off, on = tdm_twins(teams, E, 3, time_limit=0.25)
    acts = tdm_random_actions(K, E, N, 9)
    ref = tdm_loop(off, acts)
    for fields in (TKEYS, ("mask", "done", "winner")):
        go = GuardedOutputs(on, fields, n_steps=K)
        _abi.check(on.L.macm_tdm_rollout_traj(on.h, ctypes.c_void_p(acts.data_ptr()), K, go.ref(), on._stream()),
                   "macm_tdm_rollout_traj")
        go.assert_equal(ref, f"TDM {fields}")
        assert_tdm_state(off, on)
        if fields is TKEYS:
            ref = tdm_loop(off, acts)


# ---- 10. a placed world has no device streams --------------------------------------------------------
def test_placed_world_with_autoreset_is_refused():
    E, N = 2, 8
    vec = FlockVec(E, n_agents=[N], seed=1, device="cuda:0", autoreset=True)
    vec.world.place(np.zeros((E, N, 2), np.float32) + np.arange(N)[None, :, None] * 2,
                    np.zeros((E, N), np.float32), np.ones((E, 1, 2), np.float32))
    before = vec.get_state()
    acts = flock_actions(3, E, N, 1)
    for call in (lambda: vec.step(acts[0]), lambda: vec.rollout(acts), lambda: vec.rollout(acts, trajectory=True),
                 lambda: vec.rollout_bots(acts[0].clone(), 3)):
        with pytest.raises(MacmError, match="placed, not reset"):
            call()
    after = vec.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    w = TdmWorld(tdm_config([4, 4]), E, device="cuda:0", autoreset=True)
    w.reset(1)
    st = w.get_state()
    w.place(st["pos"], st["angle"])
    before = w.get_state()
    ta = tdm_random_actions(3, E, 8, 1)
    for call in (lambda: w.step(ta[0]), lambda: w.rollout(ta), lambda: w.rollout_traj(ta),
                 lambda: w.rollout_bots(ta[0].clone(), 3)):
        with pytest.raises(MacmError, match="placed, not reset"):
            call()
    after = w.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)


# ---- 11. off after on ---------------------------------------------------------------------------------
def test_autoreset_off_after_on():
    """set_autoreset(0) restores today's results: the rollout steps past done as a never-enabled twin."""
    E, N, K = 8, 64, 20
    never = FlockVec(E, n_agents=[N], seed=37, device="cuda:0", time_limit=0.25)
    b = FlockVec(E, n_agents=[N], seed=37, device="cuda:0", time_limit=0.25)
    b.world.set_autoreset(True)
    b.world.set_autoreset(False)
    acts = flock_actions(K, E, N, 71)
    ta = never.rollout(acts, trajectory=True)
    tb = b.rollout(acts, trajectory=True)
    assert_traj(ta, tb, "never enabled vs switched off")
    assert bool(tb["done"][15:].all()) and int(b.get_state()["step_count"].min()) == K
    assert_same(never, b, "off after on")
    t1 = TdmWorld(tdm_config([4, 4], time_limit=0.25), E, device="cuda:0")
    t2 = TdmWorld(tdm_config([4, 4], time_limit=0.25), E, device="cuda:0", autoreset=True)
    t2.set_autoreset(False)
    t1.reset(5)
    t2.reset(5)
    assert t1.launch_flags() == t2.launch_flags()
    ta = tdm_random_actions(K, E, 8, 2)
    assert_traj(t1.rollout_traj(ta), t2.rollout_traj(ta), "TDM off after on")
    assert_tdm_state(t1, t2)
