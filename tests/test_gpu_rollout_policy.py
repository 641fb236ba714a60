"""macm_world_rollout_policy / _traj: the closed loop step -> policy -> step in one launch on the wave
path (env_rollout_w64 / env_rollout_ar_w64 with the MLP of policy_mlp.hpp where the bot is), as the
launches of the loop on the workgroup path.

The bar: a twin world with the same seed, driven by the loop `step -> macm_policy_flock` (with autoreset:
`step -> capture final -> reset_envs(done) -> macm_policy_flock`), gives every trajectory row, every
action row, every logits row, the final get_state, the counters, the reward sums and the final outputs
bit for bit; one case also equals the oracle driven by tests/policy_ref.py. Every buffer the launch
writes sits between guard bands."""
import ctypes

import numpy as np
import pytest
import torch

import policy_ref as pr
from guard_bands import Guarded, GuardedOutputs
from parity import assert_state_equal, oracle_for
from test_gpu_final_outputs import Capture, FinalBufs, flock_step_cap
from test_gpu_rollout_autoreset import FKEYS, assert_flock_end, flock_twins

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.policy import MlpPolicy  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

DEV = "cuda:0"
F64C = {"obs_dtype": torch.float64, "coord": "cartesian"}


def seeded_policy(od, H=32, nh=2, seed=pr.WEIGHT_SEED):
    pol = MlpPolicy(od, H, nh, DEV)
    pol.params.copy_(torch.from_numpy(pr.seeded_params(od, H, nh, seed)))
    return pol


def noise_rows(K, E, N, seed=5):
    return torch.from_numpy(pr.gumbel_noise((K, E, N, 9), seed)).to(DEV)


def policy_loop(vec, pol, act0, K, noise, cap=None):
    """The twin's loop; returns the trajectory, the K + 1 action rows and the K logits rows."""
    w = vec.world
    act = act0.clone()
    rows, arows, lrows = [], [act.clone()], []
    for k in range(K):
        if cap is not None:
            rows.append(flock_step_cap(vec, act, cap, k))  # step -> capture -> reset_envs(done)
        else:
            w.step(act)
            rows.append({f: getattr(w, f).clone() for f in FKEYS})
        lg = torch.empty((w.E, w.N, 9), dtype=torch.float32, device=DEV)
        pol.act(w.obs, noise=None if noise is None else noise[k], logits=lg, out=act)
        arows.append(act.clone())
        lrows.append(lg)
    return {f: torch.stack([r[f] for r in rows]) for f in FKEYS}, torch.stack(arows), torch.stack(lrows)


def launch(vec, act0, K, noise, traj, with_logits, fields=FKEYS):
    """One call through the C-ABI into guarded buffers; (outputs, action rows, logits rows or None)."""
    w = vec.world
    E, N = w.E, w.N
    acts = Guarded((K + 1, E, N, 3) if traj else (E, N, 3), torch.uint8, DEV)
    if traj:
        acts.t[0] = act0
    else:
        acts.t.copy_(act0)
    lg = Guarded((K, E, N, 9) if traj else (E, N, 9), torch.float32, DEV) if with_logits else None
    go = GuardedOutputs(w, fields, n_steps=K if traj else None)
    fn = w.L.macm_world_rollout_policy_traj if traj else w.L.macm_world_rollout_policy
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _abi.check(fn(w.h, p(acts.t), K, p(noise), p(lg.t) if lg else None, go.ref(), w._stream()), fn.__name__)
    torch.cuda.synchronize()
    go.check_bands("policy rollout")
    assert acts.bands_intact(), "a store outside the actions buffer"
    assert lg is None or lg.bands_intact(), "a store outside the logits buffer"
    return go, acts.t, (lg.t if lg else None)


def compare(ref, arows, lrows, go, acts, lg, K, traj, ctx):
    if traj:
        go.assert_equal(ref, ctx)
        assert torch.equal(acts, arows), f"{ctx}: action rows"
        if lg is not None:
            assert torch.equal(lg.view(torch.int32), lrows.view(torch.int32)), f"{ctx}: logits rows"
    else:
        go.assert_equal({f: ref[f][K - 1] for f in ref}, ctx)
        assert torch.equal(acts, arows[K]), f"{ctx}: the policy's next actions"
        if lg is not None:
            assert torch.equal(lg.view(torch.int32), lrows[K - 1].view(torch.int32)), f"{ctx}: the last logits"


FORMS = [(t, n, l) for t in (True, False) for n in (True, False) for l in (True, False)]
FORM_IDS = [f"{'traj' if t else 'over'}-{'noise' if n else 'argmax'}-{'logits' if l else 'nologits'}" for t, n, l in FORMS]


# ---- 1. the wave path: every instantiation, both forms, noise and logits given or NULL ---------------
@pytest.mark.parametrize("traj,with_noise,with_logits", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("E,N,K,kw", [
    (8, 3, 7, {}),
    (8, 31, 8, {}),
    (8, 33, 9, {}),
    (16, 64, 12, {}),
    (16, 64, 33, {}),    # K >= 32: the envs in the balanced order
    (2048, 64, 3, {}),   # >= 2048 envs: the scalar-sweep instantiations
    (8, 64, 6, F64C),
], ids=["8x3", "8x31", "8x33", "16x64", "16x64x33", "2048x64", "8x64f64cart"])
def test_wave_launch_equals_the_loop(E, N, K, kw, traj, with_noise, with_logits):
    off, on = FlockVec(E, n_agents=[N], seed=11, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=11, device=DEV, **kw)
    pol = seeded_policy(on.world.OD)
    on.set_policy(pol)
    noise = noise_rows(K, E, N) if with_noise else None
    act0 = pol.act(off.obs)
    ref, arows, lrows = policy_loop(off, pol, act0, K, noise)
    go, acts, lg = launch(on, act0, K, noise, traj, with_logits)
    compare(ref, arows, lrows, go, acts, lg, K, traj, f"{E} x {N} x {K}")
    assert_flock_end(off, on, "after the launch", outputs=False)
    if with_noise:
        assert len(torch.unique(arows)) == 3, "the decisions differ"


# ---- 2. the other hidden shapes inside the launch -----------------------------------------------------
@pytest.mark.parametrize("H,nh", [(16, 1), (16, 2), (32, 1)])
@pytest.mark.parametrize("N,kw", [(64, {}), (20, F64C)], ids=["64polar", "20f64cart"])
def test_wave_launch_hidden_shapes(N, kw, H, nh):
    E, K = 8, 6
    off, on = FlockVec(E, n_agents=[N], seed=3, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=3, device=DEV, **kw)
    pol = seeded_policy(on.world.OD, H, nh)
    on.set_policy(pol)
    noise = noise_rows(K, E, N)
    act0 = pol.act(off.obs)
    ref, arows, lrows = policy_loop(off, pol, act0, K, noise)
    go, acts, lg = launch(on, act0, K, noise, True, True)
    compare(ref, arows, lrows, go, acts, lg, K, True, f"H {H} x {nh}")
    assert_flock_end(off, on, f"H {H} x {nh}", outputs=False)


# ---- 3. autoreset: every env ends twice inside the launch; the final outputs -------------------------
@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("N,kw", [(64, {}), (20, F64C), (2048, {})], ids=["64", "20f64cart", "scal"])
def test_autoreset_inside_the_launch(N, kw, traj):
    E, K = 8, 40
    if N == 2048:  # the scalar-sweep instantiation of the autoreset kernel: 2048 envs of 64, fewer steps
        E, N, K = 2048, 64, 18
    off, on = flock_twins(E, N, 19, time_limit=0.25, **kw)  # an episode ends at its 16th step
    pol = seeded_policy(on.world.OD)
    on.set_policy(pol)
    fin = FinalBufs(on.world)
    cap = Capture(E)
    noise = noise_rows(K, E, N)
    act0 = pol.act(off.obs)
    ref, arows, lrows = policy_loop(off, pol, act0, K, noise, cap)
    go, acts, lg = launch(on, act0, K, noise, traj, True)
    compare(ref, arows, lrows, go, acts, lg, K, traj, "autoreset")
    ends = K // 16
    assert int(ref["done"].sum()) == ends * E and (cap.ends == ends).all()
    if K == 40:
        assert ends == 2, "every env ends twice inside the launch"
    fin.check(cap, "final outputs")
    assert_flock_end(off, on, "autoreset", outputs=False)
    if traj:  # the action after an end comes from the new initial obs, which row 15 of obs holds
        assert bool(go["done"][15].all())
        want = pol.act(go["obs"][15].clone(), noise=noise[15])
        assert torch.equal(acts[16], want)


# ---- 4. a spill step inside the loop ------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
def test_forced_spill_inside_the_loop(autoreset):
    E, N, K = 8, 64, 18
    kw = dict(time_limit=0.25) if autoreset else {}
    off = FlockVec(E, n_agents=[N], seed=23, device=DEV, **kw)
    on = FlockVec(E, n_agents=[N], seed=23, device=DEV, autoreset=autoreset, **kw)
    for v in (off, on):
        v.world.set_debug(_abi.DEBUG_FORCE_SPILL)
    pol = seeded_policy(4)
    on.set_policy(pol)
    noise = noise_rows(K, E, N)
    act0 = pol.act(off.obs)
    ref, arows, lrows = policy_loop(off, pol, act0, K, noise, Capture(E) if autoreset else None)
    go, acts, lg = launch(on, act0, K, noise, True, True)
    compare(ref, arows, lrows, go, acts, lg, K, True, "forced spill")
    assert on.spilled() > 0
    assert_flock_end(off, on, "forced spill", outputs=False)


# ---- 5. the learner overwrites the weights in place between two launches -----------------------------
def test_weights_overwritten_in_place_between_launches():
    E, N, K = 8, 64, 5
    off, on = FlockVec(E, n_agents=[N], seed=29, device=DEV), FlockVec(E, n_agents=[N], seed=29, device=DEV)
    pol = seeded_policy(4)
    old = seeded_policy(4)
    on.set_policy(pol)  # registered once
    ptr = pol.params.data_ptr()
    act = pol.act(off.obs)
    for i, seed in enumerate((pr.WEIGHT_SEED, 12345)):
        pol.params.copy_(torch.from_numpy(pr.seeded_params(4, 32, 2, seed)))  # in place
        assert pol.params.data_ptr() == ptr
        ref, arows, lrows = policy_loop(off, pol, act, K, None)
        go, acts, lg = launch(on, act, K, None, True, True)
        compare(ref, arows, lrows, go, acts, lg, K, True, f"launch {i}")
        act = arows[K].clone()
    # the second launch followed the new weights: the old ones give other logits on its observations
    lg_old = torch.empty_like(lg[0])
    old.act(go["obs"][0].clone(), logits=lg_old)
    assert not torch.equal(lg_old, lg[0])
    want = pr.logits_of(pr.seeded_params(4, 32, 2, 12345), 4, 32, 2, go["obs"][0].cpu().numpy())
    assert np.array_equal(want.view(np.uint32), lg[0].cpu().numpy().view(np.uint32))
    assert_flock_end(off, on, "two launches", outputs=False)


# ---- 6. the workgroup path: the launches of the loop --------------------------------------------------
@pytest.mark.parametrize("traj,with_noise,with_logits", [(True, True, True), (False, True, True), (True, False, False)],
                         ids=["traj", "over", "traj-bare"])
@pytest.mark.parametrize("autoreset", [False, True])
def test_workgroup_path(autoreset, traj, with_noise, with_logits):
    E, N, K = 4, 65, 3
    kw = dict(start_spread=12)
    if autoreset:
        kw.update(time_limit=1.5 / 60.0)  # done when 2 / 60 > time_limit: an episode ends at its 2nd step
    off = FlockVec(E, n_agents=[N], seed=31, device=DEV, **kw)
    on = FlockVec(E, n_agents=[N], seed=31, device=DEV, autoreset=autoreset, **kw)
    assert on.world.info.n_agents == 65
    pol = seeded_policy(4)
    on.set_policy(pol)
    cap = Capture(E) if autoreset else None
    fin = FinalBufs(on.world) if autoreset else None
    noise = noise_rows(K, E, N) if with_noise else None
    act0 = pol.act(off.obs)
    ref, arows, lrows = policy_loop(off, pol, act0, K, noise, cap)
    go, acts, lg = launch(on, act0, K, noise, traj, with_logits)
    compare(ref, arows, lrows, go, acts, lg, K, traj, "workgroup path")
    if autoreset:
        assert int(ref["done"].sum()) == E
        fin.check(cap, "workgroup path final outputs")
    assert_flock_end(off, on, "workgroup path", outputs=False)


# ---- 7. against the oracle driven by policy_ref ------------------------------------------------------
def test_launch_equals_the_oracle_under_policy_ref():
    """The run of test_policy_ref.py::test_reference_closed_loop_visits_every_action on the device,
    through the Python layer: the same actions, and the oracle's final state."""
    E, N, K, od, H, nh = 4, 8, 30, 4, 32, 2
    params = pr.seeded_params(od, H, nh)
    noise = pr.gumbel_noise((K, E, N, 9), 5)
    orc = oracle_for(to_config(flockSettings(), N, 1, obs_f64=True), None, E, 42)
    o_acts, o_logits, _ = pr.oracle_closed_loop(orc, params, od, H, nh, K, noise)
    vec = FlockVec(E, n_agents=[N], seed=42, device=DEV, obs_dtype=torch.float64)
    layers = [torch.nn.Linear(i, o) for i, o in pr.layer_shapes(od, H, nh)]
    ws, bs = pr.split_params(params, od, H, nh)
    with torch.no_grad():
        for lin, w, b in zip(layers, ws, bs):
            lin.weight.copy_(torch.from_numpy(w.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
    pol = MlpPolicy.from_linear_layers(layers, device=DEV)  # transposes back to [in][out]
    assert np.array_equal(pol.params.cpu().numpy(), params)
    uw, ub = pol.unpack()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(uw + ub, ws + bs))
    vec.set_policy(pol)
    acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
    acts[0] = pol.act(vec.obs)
    logits = torch.empty((K, E, N, 9), dtype=torch.float32, device=DEV)
    traj = vec.rollout_policy(acts, K, noise=torch.from_numpy(noise).to(DEV), trajectory=True, logits=logits)
    assert np.array_equal(acts.cpu().numpy(), o_acts), "the actions of the oracle's closed loop"
    # the logits are the definition's on the observations the device wrote
    want = pr.logits_of(params, od, H, nh, traj["obs"].cpu().numpy())
    assert np.array_equal(want.view(np.uint32), logits.cpu().numpy().view(np.uint32))
    np.testing.assert_allclose(logits.cpu().numpy(), o_logits, rtol=1e-4, atol=1e-4)
    assert_state_equal(vec.get_state(), orc.get_state(vec.world.C), "vs oracle")
    assert torch.equal(vec.world.obs, traj["obs"][K - 1]) and vec.status() == 0
    # the overwrite form through the Python layer: two more steps, the outputs are the world's own
    act = acts[K].clone()
    obs, nbr, rew, done = vec.rollout_policy(act, 2)
    assert obs is vec.world.obs and rew.shape == (E, N) and done.shape == (E,)
    assert (vec.get_state()["step_count"] == K + 2).all()


# ---- 8. refusals --------------------------------------------------------------------------------------
def test_refusals():
    E, N, K = 2, 8, 3
    vec = FlockVec(E, n_agents=[N], seed=1, device=DEV)
    w = vec.world
    act = torch.ones((E, N, 3), dtype=torch.uint8, device=DEV)
    before = vec.get_state()
    with pytest.raises(MacmError, match="no policy is registered"):
        vec.rollout_policy(act, K)
    pol = seeded_policy(4)
    vec.set_policy(pol)
    go = GuardedOutputs(w, ("nbr_id", "reward", "collided", "done"))  # obs NULL
    for fn in (w.L.macm_world_rollout_policy, w.L.macm_world_rollout_policy_traj):
        assert fn(w.h, ctypes.c_void_p(act.data_ptr()), K, None, None, go.ref(), w._stream()) == _abi.E_INVALID
        assert b"obs" in w.L.macm_last_error()
    vec.set_policy(None)  # cleared
    with pytest.raises(MacmError, match="no policy is registered"):
        vec.rollout_policy(act, K, trajectory=False)
    with pytest.raises(MacmError, match="in_dim") as ei:
        vec.set_policy(seeded_policy(6))  # the world is polar: 4
    assert ei.value.code == _abi.E_INVALID
    cart = FlockVec(E, n_agents=[N], seed=1, device=DEV, coord="cartesian")
    with pytest.raises(MacmError, match="in_dim"):
        cart.set_policy(pol)
    cont = FlockVec(E, n_agents=[N], seed=1, device=DEV, action_mode="continuous")
    with pytest.raises(MacmError) as ei:
        cont.set_policy(pol)
    assert ei.value.code == -4, "MACM_E_UNSUPPORTED for a continuous-action world"
    with pytest.raises(MacmError, match="no policy is registered"):  # nothing was registered by the refused calls
        cart.rollout_policy(act, K)
    torch.cuda.synchronize()
    after = vec.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    vec.set_policy(pol)
    assert vec.rollout_policy(act, 0) is not None, "n_steps = 0 does nothing"
    for k in before:
        np.testing.assert_array_equal(before[k], vec.get_state()[k], err_msg=k)
