"""macm_world_rollout_policy_value / _traj: the closed loop step -> policy -> step with the registered
critic evaluated beside the actor (the ObsPolV instantiations of env_rollout_w64 / env_rollout_ar_w64; on
the workgroup path the launches of the loop).

The bar: a twin world with the same seed, driven by the per-step loop
    step -> macm_value_flock (boot) -> [capture final -> reset_envs(done)] -> macm_policy_flock, macm_value_flock (values)
gives every values row, every boot row and everything test_gpu_rollout_policy.py compares (trajectory,
actions, logits, final state, counters, reward sums, final outputs) bit for bit. Every buffer the launch
writes sits between guard bands; row 0 of a trajectory's values is the caller's and keeps its prefill."""
import ctypes

import numpy as np
import pytest
import torch

import policy_ref as pr
import value_ref as vr
from guard_bands import Guarded, GuardedOutputs
from parity import assert_state_equal, oracle_for
from test_gpu_final_outputs import Capture, FinalBufs
from test_gpu_rollout_autoreset import FKEYS, assert_flock_end, flock_twins
from test_gpu_rollout_policy import F64C, compare, noise_rows, seeded_policy

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.policy import MlpCritic  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

DEV = "cuda:0"


def seeded_critic(od, H=32, nh=2, seed=vr.WEIGHT_SEED):
    c = MlpCritic(od, H, nh, DEV)
    c.params.copy_(torch.from_numpy(vr.seeded_params(od, H, nh, seed)))
    return c


def ibits(t):
    return t.contiguous().view(torch.int32)


def value_loop(vec, pol, crit, act0, K, noise, cap=None):
    """The twin's loop. Returns the trajectory, the K + 1 action rows, the K logits rows, the K + 1 values
    rows (row 0: V of the obs on entry) and the K boot rows. cap: a Capture, the loop of an autoreset
    world (flock_step_cap's pattern with macm_value_flock on the row that is captured)."""
    w = vec.world
    act = act0.clone()
    rows, arows, lrows, vrows, brows = [], [act.clone()], [], [crit.value(w.obs)], []
    for k in range(K):
        w.step(act)
        brows.append(crit.value(w.obs))  # the obs the step produced, before any reset
        if cap is not None:
            row = {f: getattr(w, f).clone() for f in ("reward", "collided", "done")}
            cap.take(k, row["done"], dict(obs=w.obs, nbr_id=w.nbr_id), w)
            w.reset_envs(row["done"].clone())
            row["obs"], row["nbr_id"] = w.obs.clone(), w.nbr_id.clone()
            rows.append(row)
        else:
            rows.append({f: getattr(w, f).clone() for f in FKEYS})
        lg = torch.empty((w.E, w.N, 9), dtype=torch.float32, device=DEV)
        pol.act(w.obs, noise=None if noise is None else noise[k], logits=lg, out=act)
        vrows.append(crit.value(w.obs))  # the obs the next action is taken from
        arows.append(act.clone())
        lrows.append(lg)
    ref = {f: torch.stack([r[f] for r in rows]) for f in FKEYS}
    return ref, torch.stack(arows), torch.stack(lrows), torch.stack(vrows), torch.stack(brows)


def launch(vec, act0, K, noise, traj, with_values=True, with_boot=True, with_logits=True):
    """One call through the C-ABI into guarded buffers; (outputs, action rows, logits, values, boot)."""
    w = vec.world
    E, N = w.E, w.N
    acts = Guarded((K + 1, E, N, 3) if traj else (E, N, 3), torch.uint8, DEV)
    if traj:
        acts.t[0] = act0
    else:
        acts.t.copy_(act0)
    lg = Guarded((K, E, N, 9) if traj else (E, N, 9), torch.float32, DEV) if with_logits else None
    gv = Guarded((K + 1, E, N) if traj else (E, N), torch.float32, DEV) if with_values else None
    gb = Guarded((K, E, N) if traj else (E, N), torch.float32, DEV) if with_boot else None
    go = GuardedOutputs(w, FKEYS, n_steps=K if traj else None)
    fn = w.L.macm_world_rollout_policy_value_traj if traj else w.L.macm_world_rollout_policy_value
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    g = lambda x: p(x.t) if x else None
    _abi.check(fn(w.h, p(acts.t), K, p(noise), g(lg), g(gv), g(gb), go.ref(), w._stream()), fn.__name__)
    torch.cuda.synchronize()
    go.check_bands("policy value rollout")
    for name, x in (("actions", acts), ("logits", lg), ("values", gv), ("boot", gb)):
        assert x is None or x.bands_intact(), f"a store outside the {name} buffer"
    if traj and gv is not None:
        assert gv.rows_untouched([True] + [False] * K), "values row 0 is the caller's: neither read nor written"
    return go, acts.t, (lg.t if lg else None), (gv.t if gv else None), (gb.t if gb else None)


def compare_values(vrows, brows, gv, gb, K, traj, ctx):
    if gv is not None:
        got, want = (gv[1:], vrows[1:]) if traj else (gv, vrows[K])
        assert torch.equal(ibits(got), ibits(want)), f"{ctx}: values"
    if gb is not None:
        want = brows if traj else brows[K - 1]
        assert torch.equal(ibits(gb), ibits(want)), f"{ctx}: boot"


def run_case(off, on, K, traj, with_noise=True, with_values=True, with_boot=True, pshape=(32, 2), vshape=(32, 2),
             cap=None, ctx=""):
    """Twin loop on `off`, one launch on `on`, everything compared; returns what the checks after it need."""
    E, N, od = on.world.E, on.world.N, on.world.OD
    pol, crit = seeded_policy(od, *pshape), seeded_critic(od, *vshape)
    on.set_policy(pol)
    on.set_critic(crit)
    noise = noise_rows(K, E, N) if with_noise else None
    act0 = pol.act(off.obs)
    ref, arows, lrows, vrows, brows = value_loop(off, pol, crit, act0, K, noise, cap)
    go, acts, lg, gv, gb = launch(on, act0, K, noise, traj, with_values, with_boot)
    compare(ref, arows, lrows, go, acts, lg, K, traj, ctx)
    compare_values(vrows, brows, gv, gb, K, traj, ctx)
    assert_flock_end(off, on, ctx, outputs=False)
    return dict(ref=ref, arows=arows, vrows=vrows, brows=brows, go=go, gv=gv, gb=gb, pol=pol, crit=crit, noise=noise)


FORMS = [(t, n, v, b) for t in (True, False) for n in (True, False) for v, b in ((True, True), (True, False), (False, True))]
FORM_IDS = [f"{'traj' if t else 'over'}-{'noise' if n else 'argmax'}-{'values' if v else 'novalues'}-{'boot' if b else 'noboot'}"
            for t, n, v, b in FORMS]


# ---- 1. the wave path: every instantiation, both forms, values / boot / noise given or NULL ------------
@pytest.mark.parametrize("traj,with_noise,with_values,with_boot", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("E,N,K,kw", [
    (8, 3, 7, {}),
    (8, 31, 8, {}),
    (8, 33, 9, {}),
    (16, 64, 12, {}),
    (16, 64, 33, {}),    # K >= 32: the envs in the balanced order
    (2048, 64, 3, {}),   # >= 2048 envs: the scalar-sweep instantiations
    (8, 64, 6, F64C),
], ids=["8x3", "8x31", "8x33", "16x64", "16x64x33", "2048x64", "8x64f64cart"])
def test_wave_launch_equals_the_loop(E, N, K, kw, traj, with_noise, with_values, with_boot):
    off, on = FlockVec(E, n_agents=[N], seed=11, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=11, device=DEV, **kw)
    r = run_case(off, on, K, traj, with_noise, with_values, with_boot, ctx=f"{E} x {N} x {K}")
    # no reset: the value of the next row is the bootstrap value of this one; and the values differ
    assert torch.equal(ibits(r["vrows"][1:]), ibits(r["brows"]))
    assert len(torch.unique(ibits(r["brows"]))) > E * N // 2


# ---- 2. critic shapes inside the launch, beside two actor shapes --------------------------------------
@pytest.mark.parametrize("pshape", [(32, 2), (16, 1)], ids=["actor32x2", "actor16x1"])
@pytest.mark.parametrize("vshape", [(16, 1), (16, 2), (32, 1), (32, 2)], ids=lambda s: f"critic{s[0]}x{s[1]}")
@pytest.mark.parametrize("N,kw", [(64, {}), (20, F64C)], ids=["64polar", "20f64cart"])
def test_critic_shapes_inside_the_launch(N, kw, vshape, pshape):
    E, K = 8, 6
    off, on = FlockVec(E, n_agents=[N], seed=3, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=3, device=DEV, **kw)
    run_case(off, on, K, True, pshape=pshape, vshape=vshape, ctx=f"critic {vshape} actor {pshape}")


# ---- 3-5. autoreset: the bootstrap value of every end, the value of the new initial obs ----------------
def check_end_semantics(r, cap, fin, K, E, ctx):
    """On the reference loop's own rows: at an ended row boot[k] and values[k + 1] differ in bits for some
    agent, at every other row they are equal. On the launch's: boot[k] of an env's last end is
    macm_value_flock of the registered final obs."""
    done = r["ref"]["done"].bool()  # [K, E]
    vnext, brows = ibits(r["vrows"][1:]), ibits(r["brows"])
    same = (vnext == brows).all(dim=2)  # [K, E]
    assert bool(same[~done].all()), f"{ctx}: a row that did not end: values[k + 1] is boot[k]"
    assert bool((~same[done]).all()), f"{ctx}: an ended row: V of the new initial obs is not V of the terminal obs"
    fin.check(cap, f"{ctx}: final outputs")
    if r["gb"] is not None and r["gb"].dim() == 3:
        vfin = r["crit"].value(fin["obs"].clone())  # [E, N]
        last = {e: k for k, e in cap.at}
        assert len(last) == E
        for e, k in last.items():
            assert torch.equal(ibits(r["gb"][k, e]), ibits(vfin[e])), f"{ctx}: boot[{k}, {e}] is V(final_obs)"


@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("N", [64, 31])
def test_autoreset_every_env_ends_at_its_16th_step(N, traj):
    E, K = 8, 20
    off, on = flock_twins(E, N, 19, time_limit=0.25)
    fin, cap = FinalBufs(on.world), Capture(E)
    r = run_case(off, on, K, traj, cap=cap, ctx="autoreset A")
    assert int(r["ref"]["done"].sum()) == E and bool(r["ref"]["done"][15].all()) and (cap.ends == 1).all()
    check_end_semantics(r, cap, fin, K, E, "autoreset A")
    if traj:  # values row 16 is V of the new initial obs, which row 15 of obs holds
        want = r["crit"].value(r["go"]["obs"][15].clone())
        assert torch.equal(ibits(r["gv"][16]), ibits(want))


@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("N,kw", [(64, {}), (20, F64C)], ids=["64", "20f64cart"])
def test_autoreset_three_ends_per_env_in_one_launch(N, kw, traj):
    """Every env ends at every 2nd step: three ends in 7 steps, which the per-env final obs cannot
    represent; boot holds the bootstrap value of each."""
    E, K = 8, 7
    off, on = flock_twins(E, N, 21, time_limit=1.5 / 60.0, **kw)
    fin, cap = FinalBufs(on.world), Capture(E)
    r = run_case(off, on, K, traj, cap=cap, ctx="autoreset B")
    done = r["ref"]["done"].bool()
    assert bool(done[1::2].all()) and not bool(done[0::2].any()) and (cap.ends == 3).all()
    check_end_semantics(r, cap, fin, K, E, "autoreset B")
    if traj:  # the earlier ends, which the final outputs no longer hold: V of the twin's captured rows
        assert not torch.equal(ibits(r["gb"][1]), ibits(r["gb"][5])), "the three ends have bootstrap values of their own"


# ---- 6. a spill step inside the loop ------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
def test_forced_spill_inside_the_loop(autoreset):
    E, N, K = 8, 64, 6
    kw = dict(time_limit=1.5 / 60.0) if autoreset else {}
    off = FlockVec(E, n_agents=[N], seed=23, device=DEV, **kw)
    on = FlockVec(E, n_agents=[N], seed=23, device=DEV, autoreset=autoreset, **kw)
    for v in (off, on):
        v.world.set_debug(_abi.DEBUG_FORCE_SPILL)
    run_case(off, on, K, True, cap=Capture(E) if autoreset else None, ctx="forced spill")
    assert on.spilled() > 0


# ---- 7. the learner overwrites the critic's params in place between two launches -----------------------
def test_critic_params_overwritten_in_place_between_launches():
    E, N, K = 8, 64, 5
    off, on = FlockVec(E, n_agents=[N], seed=29, device=DEV), FlockVec(E, n_agents=[N], seed=29, device=DEV)
    pol, crit, old = seeded_policy(4), seeded_critic(4), seeded_critic(4)
    on.set_policy(pol)
    on.set_critic(crit)  # registered once
    ptr = crit.params.data_ptr()
    act = pol.act(off.obs)
    for i, seed in enumerate((vr.WEIGHT_SEED, 4321)):
        crit.params.copy_(torch.from_numpy(vr.seeded_params(4, 32, 2, seed)))  # in place
        assert crit.params.data_ptr() == ptr
        ref, arows, lrows, vrows, brows = value_loop(off, pol, crit, act, K, None)
        go, acts, lg, gv, gb = launch(on, act, K, None, True)
        compare(ref, arows, lrows, go, acts, lg, K, True, f"launch {i}")
        compare_values(vrows, brows, gv, gb, K, True, f"launch {i}")
        act = arows[K].clone()
    # the second launch followed the new params: the old ones give other values on its observations
    assert not torch.equal(ibits(old.value(go["obs"][0].clone())), ibits(gb[0]))
    want = vr.value_of(vr.seeded_params(4, 32, 2, 4321), 4, 32, 2, go["obs"][0].cpu().numpy())
    assert pr.same_bits(gb[0].cpu().numpy(), want).all()
    assert_flock_end(off, on, "two launches", outputs=False)


# ---- 8. the workgroup path: the launches of the loop --------------------------------------------------
@pytest.mark.parametrize("traj,with_values,with_boot", [(True, True, True), (False, True, True), (True, True, False),
                                                        (True, False, True)],
                         ids=["traj", "over", "traj-values", "traj-boot"])
@pytest.mark.parametrize("autoreset", [False, True])
def test_workgroup_path(autoreset, traj, with_values, with_boot):
    E, N, K = 4, 65, 3
    kw = dict(start_spread=12)
    if autoreset:
        kw.update(time_limit=1.5 / 60.0)  # an episode ends at its 2nd step
    off = FlockVec(E, n_agents=[N], seed=31, device=DEV, **kw)
    on = FlockVec(E, n_agents=[N], seed=31, device=DEV, autoreset=autoreset, **kw)
    assert on.world.info.n_agents == 65
    cap = Capture(E) if autoreset else None
    fin = FinalBufs(on.world) if autoreset else None
    r = run_case(off, on, K, traj, True, with_values, with_boot, cap=cap, ctx="workgroup path")
    if autoreset:
        assert int(r["ref"]["done"].sum()) == E
        check_end_semantics(r, cap, fin, K, E, "workgroup path")


# ---- 9. against the oracle driven by policy_ref, the critic by value_ref ------------------------------
def test_launch_equals_the_oracle_under_the_references():
    E, N, K, od = 4, 16, 12, 4
    pshape, vshape = (32, 2), (16, 2)
    pparams, vparams = pr.seeded_params(od, *pshape), vr.seeded_params(od, *vshape)
    noise = pr.gumbel_noise((K, E, N, 9), 5)
    orc = oracle_for(to_config(flockSettings(), N, 1, obs_f64=True), None, E, 42)
    o_obs0, _ = orc.observe()
    o_acts, _, results = pr.oracle_closed_loop(orc, pparams, od, *pshape, K, noise)
    o_obs = np.stack([r["obs"] for r in results])  # [K, E, N, od]: the oracle's observations
    vec = FlockVec(E, n_agents=[N], seed=42, device=DEV, obs_dtype=torch.float64)
    pol, crit = seeded_policy(od, *pshape), seeded_critic(od, *vshape)
    vec.set_policy(pol)
    vec.set_critic(crit)
    acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
    acts[0] = pol.act(vec.obs)
    vals = torch.empty((K + 1, E, N), dtype=torch.float32, device=DEV)
    vals[0] = crit.value(vec.obs)
    boot = torch.empty((K, E, N), dtype=torch.float32, device=DEV)
    traj = vec.rollout_policy(acts, K, noise=torch.from_numpy(noise).to(DEV), trajectory=True, values=vals, boot=boot)
    assert np.array_equal(acts.cpu().numpy(), o_acts), "the actions of the oracle's closed loop"
    assert_state_equal(vec.get_state(), orc.get_state(vec.world.C), "vs oracle")
    # bit for bit the definition on the observations the device wrote
    want = vr.value_of(vparams, od, *vshape, traj["obs"].cpu().numpy())
    assert pr.same_bits(boot.cpu().numpy(), want).all() and pr.same_bits(vals[1:].cpu().numpy(), want).all()
    # and value_ref on the oracle's observations. A float64 obs of the device is within a few float64 ulp
    # of the oracle's (test_gpu_parity.obs_check), so its float32 rounding differs by one float32 ulp at
    # most, 2^-23 relative on inputs below 2^6; the seeded layers have gains below 1, so 1e-4 is orders
    # above what can arise (the bound test_gpu_rollout_policy.py uses for the logits).
    o_val = vr.value_of(vparams, od, *vshape, o_obs)
    np.testing.assert_allclose(boot.cpu().numpy(), o_val, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(vals[1:].cpu().numpy(), o_val, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(vals[0].cpu().numpy(), vr.value_of(vparams, od, *vshape, o_obs0), rtol=1e-4, atol=1e-4)
    assert len(np.unique(o_val.view(np.uint32))) > K * E * N // 2
    # the overwrite form through the Python layer: two more steps
    act = acts[K].clone()
    v2, b2 = torch.empty((E, N), dtype=torch.float32, device=DEV), torch.empty((E, N), dtype=torch.float32, device=DEV)
    obs, nbr, rew, done = vec.rollout_policy(act, 2, values=v2, boot=b2)
    assert obs is vec.world.obs and (vec.get_state()["step_count"] == K + 2).all()
    assert torch.equal(ibits(v2), ibits(crit.value(obs))) and torch.equal(ibits(b2), ibits(v2))


# ---- 10. a registered critic changes nothing else ------------------------------------------------------
def test_a_registered_critic_leaves_the_other_rollouts_alone():
    E, N, K = 8, 64, 6
    plain, withc = FlockVec(E, n_agents=[N], seed=37, device=DEV), FlockVec(E, n_agents=[N], seed=37, device=DEV)
    pol = seeded_policy(4)
    for v in (plain, withc):
        v.set_policy(pol)
    withc.set_critic(seeded_critic(4))
    noise = noise_rows(K, E, N)
    outs = []
    for v in (plain, withc):
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        acts[0] = pol.act(v.obs)
        lg = torch.empty((K, E, N, 9), dtype=torch.float32, device=DEV)
        t = v.rollout_policy(acts, K, noise=noise, trajectory=True, logits=lg)
        outs.append((acts, lg, {f: t[f].clone() for f in FKEYS}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(ibits(outs[0][1]), ibits(outs[1][1]))
    for f in FKEYS:
        assert torch.equal(outs[0][2][f], outs[1][2][f]), f
    assert_flock_end(plain, withc, "rollout_policy with a critic registered", outputs=False)
    bots = []
    for v in (plain, withc):
        act = outs[0][0][K].clone()
        v.rollout_bots(act, K)
        bots.append((act, {f: getattr(v.world, f).clone() for f in FKEYS}))
    assert torch.equal(bots[0][0], bots[1][0])
    for f in FKEYS:
        assert torch.equal(bots[0][1][f], bots[1][1][f]), f
    assert_flock_end(plain, withc, "rollout_bots with a critic registered", outputs=False)
    withc.set_critic(None)  # cleared: the value entry point is refused again
    with pytest.raises(MacmError, match="no critic is registered"):
        withc.rollout_policy(outs[0][0][K].clone(), 1, values=torch.empty((E, N), dtype=torch.float32, device=DEV))


# ---- 11. refusals --------------------------------------------------------------------------------------
def test_refusals():
    E, N, K = 2, 8, 3
    vec = FlockVec(E, n_agents=[N], seed=1, device=DEV)
    w = vec.world
    act = torch.ones((E, N, 3), dtype=torch.uint8, device=DEV)
    vals, boot = Guarded((E, N), torch.float32, DEV), Guarded((E, N), torch.float32, DEV)
    before = vec.get_state()
    pol, crit = seeded_policy(4), seeded_critic(4)
    vec.set_policy(pol)
    with pytest.raises(MacmError, match="no critic is registered") as ei:
        vec.rollout_policy(act, K, values=vals.t, boot=boot.t)
    assert ei.value.code == _abi.E_INVALID
    vec.set_policy(None)
    vec.set_critic(crit)
    with pytest.raises(MacmError, match="no policy is registered"):
        vec.rollout_policy(act, K, values=vals.t)
    vec.set_policy(pol)
    go = GuardedOutputs(w, FKEYS)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for fn in (w.L.macm_world_rollout_policy_value, w.L.macm_world_rollout_policy_value_traj):
        assert fn(w.h, p(act), K, None, None, None, None, go.ref(), w._stream()) == _abi.E_INVALID
        assert b"both NULL" in w.L.macm_last_error()
    noobs = GuardedOutputs(w, ("nbr_id", "reward", "collided", "done"))
    assert w.L.macm_world_rollout_policy_value(w.h, p(act), K, None, None, p(vals.t), None, noobs.ref(),
                                               w._stream()) == _abi.E_INVALID
    assert b"obs" in w.L.macm_last_error()
    with pytest.raises(MacmError, match="in_dim") as ei:
        vec.set_critic(seeded_critic(6))  # the world is polar: 4
    assert ei.value.code == _abi.E_INVALID
    for bad in (dict(hidden=8), dict(n_hidden=3), dict(reserved=1), dict(params=None), dict(params=crit.params.data_ptr() + 4)):
        kw = dict(in_dim=4, hidden=32, n_hidden=2, reserved=0, params=crit.params.data_ptr())
        kw.update(bad)
        s = _abi.MacmValueMlp(kw["in_dim"], kw["hidden"], kw["n_hidden"], kw["reserved"],
                              ctypes.c_void_p(kw["params"]) if kw["params"] else None)
        assert w.L.macm_world_set_critic(w.h, ctypes.byref(s)) == _abi.E_INVALID, bad
    cart = FlockVec(E, n_agents=[N], seed=1, device=DEV, coord="cartesian")
    with pytest.raises(MacmError, match="in_dim"):
        cart.set_critic(crit)
    cont = FlockVec(E, n_agents=[N], seed=1, device=DEV, action_mode="continuous")
    with pytest.raises(MacmError) as ei:
        cont.set_critic(crit)
    assert ei.value.code == -4, "MACM_E_UNSUPPORTED for a continuous-action world"
    with pytest.raises(ValueError, match="values must be"):
        vec.rollout_policy(act, K, values=torch.empty((K, E, N), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="boot must be"):
        vec.rollout_policy(act, K, boot=boot.t.double())
    torch.cuda.synchronize()
    after = vec.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    # the refused set_critic calls left the registration alone; n_steps = 0 does nothing
    assert vec.rollout_policy(act, 0, values=vals.t, boot=boot.t) is not None
    for k in before:
        np.testing.assert_array_equal(before[k], vec.get_state()[k], err_msg=k)
    assert vals.rows_untouched(np.ones(E, bool)) and boot.rows_untouched(np.ones(E, bool)), "nothing was stored"
    vec.rollout_policy(act, 1, values=vals.t, boot=boot.t)
    assert torch.equal(ibits(vals.t), ibits(crit.value(w.obs))) and vals.bands_intact() and boot.bands_intact()
