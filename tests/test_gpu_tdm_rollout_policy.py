"""macm_tdm_rollout_policy / _traj: the closed loop step -> actor -> step in one launch on the wave path
(env_rollout_w64 / env_rollout_ar_w64 with the set policy of tdm_policy.hpp where the bot is, for the
lanes of the policy's teams), as the launches of the loop on the workgroup path.

The bar is test_gpu_rollout_policy.py's: a twin world with the same seed, driven by the per-step loop
`step -> [capture, reset_envs(done)] -> combat_actions (the bot teams) -> TdmSetPolicy.act(agents=)`,
gives every trajectory row, action row, logits row and hit_id row, the final get_state, counters,
spilled, status and final outputs bit for bit. Every buffer the launch writes sits between guard bands;
the logits rows of bot-driven agents keep their prefill on both sides."""
import ctypes

import numpy as np
import pytest
import torch

import tdm_policy_ref as ref
from guard_bands import Guarded, GuardedOutputs
from oracle import OracleTDM
from parity import combat_bot
from test_gpu_final_outputs import Capture, FinalBufs
from test_gpu_tdm import assert_tdm_state_equal

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.tdm_policy import TdmSetPolicy  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402

DEV = "cuda:0"
TKEYS = TdmWorld._TRAJ_KEYS
NL = ref.N_LOGITS


def seeded_policy(H=32, seed=ref.WEIGHT_SEED):
    pol = TdmSetPolicy(H, DEV)
    pol.params.copy_(torch.from_numpy(ref.seeded_params(H, seed)))
    return pol


def noise_rows(K, E, N, seed=5):
    return torch.from_numpy(ref.gumbel_noise((K, E, N, NL), seed)).to(DEV)


def twins(teams, E, seed, autoreset=False, events=False, spill=False, obs_f64=False, **cfg):
    """(the loop's world: autoreset off, the launch's world), the same seed"""
    off = TdmWorld(tdm_config(teams, obs_f64=obs_f64, **cfg), E, device=DEV, events=events)
    on = TdmWorld(tdm_config(teams, obs_f64=obs_f64, **cfg), E, device=DEV, autoreset=autoreset, events=events)
    for w in (off, on):
        w.reset(seed)
        if spill:
            w.set_debug(_abi.DEBUG_FORCE_SPILL)
    return off, on


def first_actions(w, pol, teams):
    """The loop's first actions from the initial obs: the bot everywhere, the policy's teams over it."""
    act = combat_actions(w.obs, w.mask)
    pol.act(w.obs, w.mask, w.health, out=act, agents=w.policy_agents(teams))
    return act


def policy_loop(w, pol, teams, act0, K, noise, reset=False, cap=None):
    """The twin's loop; the trajectory (hit_id too with events on), the K + 1 action rows, the K logits rows."""
    agents = w.policy_agents(teams)
    every = bool(agents.all())
    act = act0.clone()
    rows, arows, lrows = [], [act.clone()], []
    for k in range(K):
        w.step(act)
        row = {f: getattr(w, f).clone() for f in ("health", "alive", "done", "winner")}  # terminal
        if w.hit_id is not None:
            row["hit_id"] = w.hit_id.clone()
        if reset:
            if cap is not None:
                cap.take(k, row["done"], dict(obs=w.obs, mask=w.mask), w)
            w.reset_envs(row["done"].clone())  # the world's health output: init_health in the reset envs
        row["obs"], row["mask"] = w.obs.clone(), w.mask.clone()
        rows.append(row)
        if not every:
            combat_actions(w.obs, w.mask, out=act)
        lg = Guarded((w.E, w.N, NL), torch.float32, DEV)  # prefilled: a bot-driven agent's row stays so
        pol.act(w.obs, w.mask, w.health, noise=None if noise is None else noise[k], logits=lg.t, out=act,
                agents=None if every else agents)
        arows.append(act.clone())
        lrows.append(lg.t.clone())
    return {f: torch.stack([r[f] for r in rows]) for f in rows[0]}, torch.stack(arows), torch.stack(lrows)


def launch(w, act0, K, noise, traj, with_logits=True, fields=TKEYS):
    """One call through the C-ABI into guarded buffers; (outputs, action rows, logits rows or None, hit rows or None)"""
    E, N = w.E, w.N
    acts = Guarded((K + 1, E, N, 4) if traj else (E, N, 4), torch.uint8, DEV)
    if traj:
        acts.t[0] = act0
    else:
        acts.t.copy_(act0)
    lg = Guarded((K, E, N, NL) if traj else (E, N, NL), torch.float32, DEV) if with_logits else None
    go = GuardedOutputs(w, fields, n_steps=K if traj else None)
    hit = None
    if w.hit_id is not None:
        hit = Guarded((K, E, N) if traj else (1, E, N), torch.int32, DEV)
        w._register_events(hit.t, K if traj else 1)
    fn = w.L.macm_tdm_rollout_policy_traj if traj else w.L.macm_tdm_rollout_policy
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    try:
        _abi.check(fn(w.h, p(acts.t), K, p(noise), p(lg.t) if lg else None, go.ref(), w._stream()), fn.__name__)
        torch.cuda.synchronize()
    finally:
        if hit is not None:
            w._register_events(w.hit_id, 1)
    go.check_bands("policy rollout")
    assert acts.bands_intact(), "a store outside the actions buffer"
    assert lg is None or lg.bands_intact(), "a store outside the logits buffer"
    assert hit is None or hit.bands_intact(), "a store outside the hit_id buffer"
    return go, acts.t, (lg.t if lg else None), (hit.t if hit else None)


def i32(t):
    return t.contiguous().view(torch.int32)


def compare(rows, arows, lrows, got, K, traj, ctx):
    go, acts, lg, hit = got
    tw = {f: rows[f] for f in TKEYS}
    if traj:
        go.assert_equal(tw, ctx)
        assert torch.equal(acts, arows), f"{ctx}: action rows"
        if lg is not None:
            assert torch.equal(i32(lg), i32(lrows)), f"{ctx}: logits rows"
        if hit is not None:
            assert torch.equal(hit, rows["hit_id"]), f"{ctx}: hit_id rows"
    else:
        go.assert_equal({f: tw[f][K - 1] for f in tw}, ctx)
        assert torch.equal(acts, arows[K]), f"{ctx}: the actors' next actions"
        if lg is not None:
            assert torch.equal(i32(lg), i32(lrows[K - 1])), f"{ctx}: the last logits"
        if hit is not None:
            assert torch.equal(hit[0], rows["hit_id"][K - 1]), f"{ctx}: the last hit_id"


def assert_end(off, on, ctx):
    sa, sb = off.get_state(), on.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{ctx}: state[{k}]")
    np.testing.assert_array_equal(off.counters(), on.counters(), err_msg=f"{ctx}: counters")
    assert off.spilled() == on.spilled(), f"{ctx}: spilled"
    assert off.status() == 0 and on.status() == 0


def run_case(teams, E, K, pol_teams, traj, H=32, noise=True, with_logits=True, seed=11, **kw):
    off, on = twins(teams, E, seed, **kw)
    pol = seeded_policy(H)
    on.set_policy(pol, pol_teams)
    nz = noise_rows(K, E, on.N) if noise else None
    act0 = first_actions(off, pol, pol_teams)
    rows, arows, lrows = policy_loop(off, pol, pol_teams, act0, K, nz, reset=kw.get("autoreset", False))
    got = launch(on, act0, K, nz, traj, with_logits)
    ctx = f"{teams} E{E} K{K} teams {pol_teams}"
    compare(rows, arows, lrows, got, K, traj, ctx)
    assert_end(off, on, ctx)
    return off, on, rows, arows, lrows, got


# ---- 1. the wave path: the instantiations, both forms, every team or team 0 against the bot ----------
@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("pol_teams", [None, [0]], ids=["all", "team0"])
@pytest.mark.parametrize("teams,E,K", [([16, 16], 8, 7), ([32, 32], 4, 6), ([3, 2], 8, 9)],
                         ids=["16v16", "32v32", "3v2"])
def test_wave_launch_equals_the_loop(teams, E, K, pol_teams, traj):
    off, on, rows, arows, lrows, got = run_case(teams, E, K, pol_teams, traj)
    a = arows[1:].cpu().numpy()
    assert set(np.unique(a[..., :3])) == {0, 1, 2} and set(np.unique(a[..., 3])) == {0, 1}, "the decisions differ"
    if pol_teams is not None and traj:  # the logits rows of the bot's team hold the prefill, the policy's do not
        n0 = teams[0]
        fill = torch.full((1,), 0xA5, dtype=torch.uint8, device=DEV).repeat(4).view(torch.float32)
        assert bool((i32(got[2][:, :, n0:]) == i32(fill)).all()) and not bool((i32(got[2][:, :, :n0]) == i32(fill)).any())


@pytest.mark.parametrize("H", [16, 32])
def test_argmax_without_logits_and_hidden_16(H):
    run_case([16, 16], 8, 5, None, True, H=H, noise=False, with_logits=False)


def test_float64_obs():
    run_case([16, 16], 8, 6, [0], True, obs_f64=True)
    run_case([32, 32], 4, 5, None, False, obs_f64=True)


# ---- 2. 12 steps in one launch equal launches of 5 + 7 -----------------------------------------------
def test_a_launch_of_12_equals_5_plus_7():
    teams, E, N = [16, 16], 8, 32
    pol = seeded_policy()
    one = TdmWorld(tdm_config(teams), E, device=DEV)
    two = TdmWorld(tdm_config(teams), E, device=DEV)
    for w in (one, two):
        w.reset(13)
        w.set_policy(pol, [0])
    nz = noise_rows(12, E, N)
    act0 = first_actions(one, pol, [0])
    g1 = launch(one, act0, 12, nz, True)
    ga = launch(two, act0, 5, nz[:5].contiguous(), True)
    gb = launch(two, ga[1][5].clone(), 7, nz[5:].contiguous(), True)
    assert torch.equal(g1[1], torch.cat([ga[1], gb[1][1:]])), "action rows"
    assert torch.equal(i32(g1[2]), i32(torch.cat([ga[2], gb[2]]))), "logits rows"
    for f in TKEYS:
        assert torch.equal(g1[0][f], torch.cat([ga[0][f], gb[0][f]])), f
    assert_end(one, two, "12 = 5 + 7")


# ---- 3. the learner overwrites the params in place between two launches ------------------------------
def test_params_overwritten_in_place_between_launches():
    teams, E, K = [16, 16], 8, 5
    off, on = twins(teams, E, 29)
    pol = seeded_policy()
    on.set_policy(pol)  # registered once
    ptr = pol.params.data_ptr()
    act = first_actions(off, pol, None)
    for i, seed in enumerate((ref.WEIGHT_SEED, 12345)):
        pol.params.copy_(torch.from_numpy(ref.seeded_params(32, seed)))  # in place
        assert pol.params.data_ptr() == ptr
        rows, arows, lrows = policy_loop(off, pol, None, act, K, None)
        got = launch(on, act, K, None, True)
        compare(rows, arows, lrows, got, K, True, f"launch {i}")
        act = arows[K].clone()
    # the second launch followed the new params: its logits are the definition's at them, on its observations
    go, _, lg, _ = got
    want = ref.logits_of(ref.seeded_params(32, 12345), 32, go["obs"][0].cpu().numpy(), go["mask"][0].cpu().numpy(),
                         go["health"][0].cpu().numpy())
    assert ref.same_bits(lg[0].cpu().numpy(), want).all()
    old = ref.logits_of(ref.seeded_params(32), 32, go["obs"][0].cpu().numpy(), go["mask"][0].cpu().numpy(),
                        go["health"][0].cpu().numpy())
    assert not ref.same_bits(old, want).all()
    assert_end(off, on, "two launches")


# ---- 4. the spill step inside the loop; events, and a twin without them ------------------------------
def test_forced_spill_inside_the_loop():
    off, on, *_ = run_case([16, 16], 8, 6, [0], True, spill=True)
    assert on.spilled() > 0


@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
def test_events_on_and_a_twin_without(traj):
    cfg = dict(world_width=8.0, world_height=8.0)
    teams, E, K = [4, 4], 8, 40
    off, on, rows, arows, lrows, got = run_case(teams, E, K, [0], traj, events=True, **cfg)
    assert bool((rows["hit_id"] >= 0).any()), "nobody was hit"
    plain = TdmWorld(tdm_config(teams, **cfg), E, device=DEV)
    plain.reset(11)
    plain.set_policy(on.policy, [0])
    gp = launch(plain, arows[0], K, noise_rows(K, E, 8), traj)
    assert gp[3] is None
    assert torch.equal(gp[1], got[1]) and torch.equal(i32(gp[2]), i32(got[2]))
    for f in TKEYS:
        assert torch.equal(gp[0][f], got[0][f]), f"without events: {f}"
    assert_end(plain, on, "events on / off")


# ---- 5. the workgroup path: the launches of the loop --------------------------------------------------
@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("teams,pol_teams", [([33, 32], [0]), ([40, 40], None)], ids=["33v32-team0", "40v40-all"])
def test_workgroup_path(teams, pol_teams, traj):
    off, on, *_ = run_case(teams, 3, 3, pol_teams, traj)
    assert on.N > 64


def test_workgroup_path_autoreset():
    teams, E, K = [33, 32], 3, 4
    off, on = twins(teams, E, 17, autoreset=True, time_limit=1.5 / 60.0)  # an episode ends at its 2nd step
    pol = seeded_policy()
    on.set_policy(pol, [1])
    fin, cap = FinalBufs(on), Capture(E)
    nz = noise_rows(K, E, on.N)
    act0 = first_actions(off, pol, [1])
    rows, arows, lrows = policy_loop(off, pol, [1], act0, K, nz, reset=True, cap=cap)
    got = launch(on, act0, K, nz, True)
    compare(rows, arows, lrows, got, K, True, "workgroup autoreset")
    assert int(rows["done"].sum()) == 2 * E
    fin.check(cap, "workgroup autoreset")
    assert_end(off, on, "workgroup autoreset")


# ---- 6. autoreset: the time limit ends every env at step 15 of 20 -------------------------------------
@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("teams,pol_teams,obs_f64", [([32, 32], None, False), ([16, 16], [0], True)],
                         ids=["32v32-all", "16v16-team0-f64"])
def test_autoreset_time_limit_ends(teams, pol_teams, obs_f64, traj):
    E, K = 4, 20
    off, on = twins(teams, E, 7, autoreset=True, obs_f64=obs_f64, time_limit=0.25)
    pol = seeded_policy()
    on.set_policy(pol, pol_teams)
    fin, cap = FinalBufs(on), Capture(E)
    nz = noise_rows(K, E, on.N)
    act0 = first_actions(off, pol, pol_teams)
    rows, arows, lrows = policy_loop(off, pol, pol_teams, act0, K, nz, reset=True, cap=cap)
    got = launch(on, act0, K, nz, traj)
    compare(rows, arows, lrows, got, K, traj, f"time limit {teams}")
    assert bool(rows["done"][15].all()) and int(rows["done"].sum()) == E
    assert (cap.ends == 1).all() and (cap.length == 16).all()
    fin.check(cap, f"time limit {teams}")
    assert_end(off, on, f"time limit {teams}")


# ---- 7. autoreset with combat ends: terminal health differs from init_health (the policy reads the latter) ----
COMBAT = ref.COMBAT_CASE  # its premises are checked on the CPU too (tests/test_tdm_policy_ref.py)


@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
def test_autoreset_combat_ends(traj):
    teams, E, seed, K, cfg = (COMBAT[k] for k in ("teams", "E", "seed", "K", "cfg"))
    # (float64 obs: the run is then the one tests/test_tdm_policy_ref.py makes with the oracle, step for step)
    off, on = twins(teams, E, seed, autoreset=True, events=True, obs_f64=True, **cfg)
    pol = seeded_policy()
    on.set_policy(pol, [0])
    fin, cap = FinalBufs(on), Capture(E)
    nz = noise_rows(K, E, 8)
    act0 = first_actions(off, pol, [0])
    rows, arows, lrows = policy_loop(off, pol, [0], act0, K, nz, reset=True, cap=cap)
    # the conditions under which a policy that read the step's health output would decide otherwise
    done = rows["done"].cpu().numpy().astype(bool)
    winner, health = rows["winner"].cpu().numpy(), rows["health"].cpu().numpy()
    ks, es = np.nonzero(done)
    assert len(ks) > 0 and (winner[ks, es] >= 0).any(), "no episode ended by combat"
    assert len(set(ks.tolist())) > 1, "the episodes end at one step only"
    # ... among the policy's agents (team 0: the first four)
    diff = [(int(k), int(e)) for k, e in zip(ks, es) if (health[k, e, :4] != on.cfg.init_health).any()]
    assert diff, "no reset env whose terminal health differs from init_health"
    got = launch(on, act0, K, nz, traj)
    compare(rows, arows, lrows, got, K, traj, "combat ends")
    fin.check(cap, "combat ends")
    assert_end(off, on, "combat ends")
    if traj:
        # the decision after an end is the definition's on the new initial obs and init_health, not on the
        # terminal health that the health row of that step holds
        k, e = diff[0]
        o, m = got[0]["obs"][k, e].cpu().numpy(), got[0]["mask"][k, e].cpu().numpy()
        want = ref.logits_of(ref.seeded_params(32), 32, o, m, np.full(8, on.cfg.init_health))
        assert ref.same_bits(got[2][k, e, :4].cpu().numpy(), want[:4]).all()
        term = ref.logits_of(ref.seeded_params(32), 32, o, m, health[k, e])
        assert not ref.same_bits(term[:4], want[:4]).all()
        # the oracle driven through the same actions ends in the same state; and its own closed loop under
        # tests/tdm_policy_ref.py (float64 obs on both sides) takes the same actions
        orc = OracleTDM(tdm_config(teams, obs_f64=True, **cfg), E, seed)
        for a in got[1][:K].cpu().numpy():
            r = orc.step(a)
            if r["done"].any():
                orc.reset_envs(r["done"])
        assert_tdm_state_equal(on.get_state(), orc.get_state(), "vs oracle")
        orc2 = OracleTDM(tdm_config(teams, obs_f64=True, **cfg), E, seed)
        o_acts, _ = ref.oracle_closed_loop(orc2, combat_bot, ref.seeded_params(32), 32, np.arange(8) < 4, K,
                                           nz.cpu().numpy(), on.cfg.init_health)
        assert np.array_equal(got[1].cpu().numpy(), o_acts), "the actions of the oracle's closed loop"


# ---- 8. refusals ----------------------------------------------------------------------------------------
def test_refusals():
    teams, E, K = [3, 2], 2, 3
    w = TdmWorld(tdm_config(teams), E, device=DEV)
    w.reset(1)
    act = torch.ones((E, 5, 4), dtype=torch.uint8, device=DEV)
    before = w.get_state()
    with pytest.raises(MacmError, match="no policy is registered"):
        w.rollout_policy(act, K)
    pol = seeded_policy()
    for tm in (0, 4, 8, 1 << 31):
        assert w.L.macm_tdm_set_policy(w.h, ctypes.byref(pol.struct()), tm) == _abi.E_INVALID
        assert b"team_mask" in w.L.macm_last_error()
    with pytest.raises(MacmError, match="no policy is registered"):  # nothing was registered by the refused calls
        w.rollout_policy(act, K)
    w.set_policy(pol, [1])
    go = GuardedOutputs(w, ("obs", "mask", "alive", "done", "winner"))  # health NULL
    for fn in (w.L.macm_tdm_rollout_policy, w.L.macm_tdm_rollout_policy_traj):
        assert fn(w.h, ctypes.c_void_p(act.data_ptr()), K, None, None, go.ref(), w._stream()) == _abi.E_INVALID
        assert b"health" in w.L.macm_last_error()
    go = GuardedOutputs(w, ("mask", "health", "alive", "done", "winner"))  # obs NULL
    assert w.L.macm_tdm_rollout_policy(w.h, ctypes.c_void_p(act.data_ptr()), K, None, None, go.ref(),
                                       w._stream()) == _abi.E_INVALID
    w.set_policy(None)  # cleared
    with pytest.raises(MacmError, match="no policy is registered"):
        w.rollout_policy(act, K)
    torch.cuda.synchronize()
    after = w.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    w.set_policy(pol)
    assert w.rollout_policy(act, 0) is not None, "n_steps = 0 does nothing"
    with pytest.raises(ValueError):
        w.rollout_policy(act, K, noise=torch.zeros((K, E, 5, 9), device=DEV))
    for k in before:
        np.testing.assert_array_equal(before[k], w.get_state()[k], err_msg=k)
