"""Policy rollouts of a world with sampling on (macm_world_set_sampling): the ObsPolS / ObsPolVS
instantiations of env_rollout_w64 / env_rollout_ar_w64, and on the workgroup path the loop's launches of
the sampled one-shot kernel.

The bar: a twin world with the same seed and sampling off, given macm_policy_noise's [K, E * N, 9] as
`noise`, gives every trajectory row, every action row, the logits, values and boot, the final outputs, the
final get_state, the counters and the reward sums bit for bit. Then: how the steps are cut into launches
does not matter, set_sampling(None) brings the argmax launch back, and the refusals that need a world."""
import ctypes

import numpy as np
import pytest
import torch

import sample_ref as S
import test_gpu_rollout_policy as tp
import test_gpu_rollout_value as tv
from test_gpu_rollout_autoreset import FKEYS, assert_flock_end
from test_gpu_rollout_policy import F64C, seeded_policy
from test_gpu_rollout_value import ibits, seeded_critic

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.policy import gumbel_noise  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

DEV = "cuda:0"
SEED = 0x0BAD_5EED_0123_4567  # >= 2**32
D0 = 2**32 - 3                # the launch's decisions cross the carry into hi32(d)
FINAL = ("final_obs", "final_nbr_id", "final_length", "final_ends")


def twins(E, N, seed, debug=0, **kw):
    """(the twin: sampling off, the world under test: sampling on at (SEED, D0)), the same env seed"""
    off, on = FlockVec(E, n_agents=[N], seed=seed, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=seed, device=DEV, **kw)
    for v in (off, on):
        if debug:
            v.world.set_debug(debug)
    on.set_sampling(SEED, D0)
    assert off.sampling is None and on.sampling == (SEED, D0)
    return off, on


def run_case(off, on, K, traj=True, critic=True, pshape=(32, 2), ctx=""):
    """The twin's launch with the noise given, the sampling world's launch without; everything compared."""
    E, N, od = on.world.E, on.world.N, on.world.OD
    pol, crit = seeded_policy(od, *pshape), seeded_critic(od)
    for v in (off, on):
        v.set_policy(pol)
        if critic:
            v.set_critic(crit)
    d0 = on.sampling[1]
    noise = gumbel_noise(SEED, d0, K, (E, N), DEV)
    assert torch.equal(off.obs, on.obs)
    act0 = pol.act(off.obs, seed=SEED, decision=d0 - 1)  # the decision before the launch's first
    if critic:
        a = tv.launch(off, act0, K, noise, traj)
        b = tv.launch(on, act0, K, None, traj)
    else:
        a = tp.launch(off, act0, K, noise, traj, True) + (None, None)
        b = tp.launch(on, act0, K, None, traj, True) + (None, None)
    (go_a, acts_a, lg_a, gv_a, gb_a), (go_b, acts_b, lg_b, gv_b, gb_b) = a, b
    go_b.assert_equal({f: go_a[f] for f in FKEYS}, ctx)
    assert torch.equal(acts_a, acts_b), f"{ctx}: action rows"
    assert torch.equal(ibits(lg_a), ibits(lg_b)), f"{ctx}: logits"
    if critic:
        lo = 1 if traj else 0
        assert torch.equal(ibits(gv_a[lo:]), ibits(gv_b[lo:])), f"{ctx}: values"
        assert torch.equal(ibits(gb_a), ibits(gb_b)), f"{ctx}: boot"
    for f in FINAL:
        x, y = getattr(off.world, f), getattr(on.world, f)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), f"{ctx}: {f}"
    assert_flock_end(off, on, ctx, outputs=False)
    assert on.sampling == (SEED, d0 + K) and off.sampling is None, f"{ctx}: the world's decision advanced by n_steps"
    assert len(torch.unique(acts_b)) == 3, f"{ctx}: the decisions differ"
    # the draws decide: the argmax of the last logits is another set of actions
    last_obs = go_b["obs"][-1] if traj else go_b["obs"]
    assert not torch.equal(pol.act(last_obs.clone()), acts_b[-1] if traj else acts_b), f"{ctx}: the actions are the argmax's"
    return dict(go=go_b, acts=acts_b, logits=lg_b, done=go_b["done"])


WORLDS = [(8, 8, {}), (5, 33, F64C), (4, 64, {})]
WORLD_IDS = ["8x8polar", "5x33f64cart", "4x64"]


# ---- 1. the wave path: every world, with and without the critic, both forms ---------------------------
@pytest.mark.parametrize("traj", [True, False], ids=["traj", "over"])
@pytest.mark.parametrize("critic", [True, False], ids=["critic", "nocritic"])
@pytest.mark.parametrize("E,N,kw", WORLDS, ids=WORLD_IDS)
def test_sampled_launch_equals_the_twin_given_the_noise(E, N, kw, critic, traj):
    off, on = twins(E, N, 11, **kw)
    run_case(off, on, 9, traj, critic, ctx=f"{E} x {N}")


# ---- 2. autoreset: two ends inside the launch; the reset env decides with the same d as noise row k ----
@pytest.mark.parametrize("critic", [True, False], ids=["critic", "nocritic"])
@pytest.mark.parametrize("E,N,kw", WORLDS, ids=WORLD_IDS)
def test_autoreset_two_ends_inside_the_launch(E, N, kw, critic):
    off, on = twins(E, N, 21, autoreset=True, final_obs=True, time_limit=1.5 / 60.0, **kw)  # an end at every 2nd step
    r = run_case(off, on, 5, True, critic, ctx=f"autoreset {E} x {N}")
    done = r["done"].bool()
    assert bool(done[1::2].all()) and not bool(done[0::2].any()) and bool((on.world.final_ends == 2).all())


# ---- 3. a spill step inside the loop -------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
def test_forced_spill_inside_the_loop(autoreset):
    kw = dict(autoreset=True, final_obs=True, time_limit=1.5 / 60.0) if autoreset else {}
    off, on = twins(4, 64, 23, debug=_abi.DEBUG_FORCE_SPILL, **kw)
    run_case(off, on, 5, ctx="forced spill")
    assert on.spilled() > 0


# ---- 4. K >= 32: rollout_sched reorders the waves; the row is the env's, not the wave's ----------------
@pytest.mark.parametrize("autoreset", [False, True])
def test_balanced_order_draws_by_env(autoreset):
    kw = dict(autoreset=True, final_obs=True, time_limit=0.25) if autoreset else {}  # an end at the 16th step
    off, on = twins(16, 64, 11, **kw)
    run_case(off, on, 33, ctx="16 x 64 x 33")


# ---- 5. the scalar-sweep instantiations (>= 2048 envs), the other net shapes ----------------------------
def test_scalar_sweep_instantiation():
    off, on = twins(2048, 64, 11)
    run_case(off, on, 2, ctx="2048 x 64")


@pytest.mark.parametrize("H,nh", [(16, 1), (16, 2), (32, 1)])
def test_hidden_shapes_inside_the_launch(H, nh):
    off, on = twins(5, 33, 3, **F64C)
    run_case(off, on, 4, pshape=(H, nh), ctx=f"H {H} x {nh}")


# ---- 6. the workgroup path: the loop calls the sampled one-shot kernel with d = decision + k ------------
@pytest.mark.parametrize("critic", [True, False], ids=["critic", "nocritic"])
@pytest.mark.parametrize("autoreset", [False, True])
def test_workgroup_path(autoreset, critic):
    kw = dict(start_spread=12)
    if autoreset:
        kw.update(autoreset=True, final_obs=True, time_limit=1.5 / 60.0)
    off, on = twins(2, 96, 31, **kw)
    assert on.world.info.n_agents == 96 and not on.world.N <= 64
    run_case(off, on, 3, True, critic, ctx="workgroup path")


# ---- 7. launch cuts do not matter ------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,kw", [(8, 8, dict(autoreset=True, time_limit=0.1)), (4, 64, {}), (2, 96, dict(start_spread=12))],
                         ids=["8x8autoreset", "4x64", "2x96wg"])
def test_launch_cuts_do_not_matter(E, N, kw):
    """K = 7 then K = 13 on one world equal K = 20 on its twin, in actions and final state (8 x 8: an episode
    lasts 0.1 s, so every env resets at least twice, on both sides of the cut)."""
    cut, whole = FlockVec(E, n_agents=[N], seed=5, device=DEV, **kw), FlockVec(E, n_agents=[N], seed=5, device=DEV, **kw)
    pol, crit = seeded_policy(cut.world.OD), seeded_critic(cut.world.OD)
    for v in (cut, whole):
        v.set_policy(pol)
        v.set_critic(crit)
        v.set_sampling(SEED, D0)
    a_cut = torch.empty((21, E, N, 3), dtype=torch.uint8, device=DEV)
    a_whole = torch.empty((21, E, N, 3), dtype=torch.uint8, device=DEV)
    a_cut[0] = a_whole[0] = pol.act(cut.obs, seed=SEED, decision=D0 - 1)
    lg_cut = torch.empty((20, E, N, 9), dtype=torch.float32, device=DEV)
    lg_whole = torch.empty_like(lg_cut)
    t1 = cut.rollout_policy(a_cut[:8], 7, trajectory=True, logits=lg_cut[:7])
    done1 = t1["done"].clone()
    assert cut.sampling == (SEED, D0 + 7)
    # the second launch takes the other entry point (with the critic): the draws do not depend on it
    vals = torch.empty((14, E, N), dtype=torch.float32, device=DEV)
    t2 = cut.rollout_policy(a_cut[7:], 13, trajectory=True, logits=lg_cut[7:], values=vals)
    t = whole.rollout_policy(a_whole, 20, trajectory=True, logits=lg_whole)
    assert cut.sampling == (SEED, D0 + 20) == whole.sampling, "get_sampling reports decision + 20"
    assert torch.equal(a_cut, a_whole), "the actions of 7 + 13 steps and of 20"
    assert torch.equal(ibits(lg_cut), ibits(lg_whole))
    assert torch.equal(torch.cat([done1, t2["done"]]), t["done"])
    if "autoreset" in kw:
        assert int(t["done"].sum()) >= 2 * E
    assert_flock_end(cut, whole, "7 + 13 against 20", outputs=False)
    # the numbers are macm_policy_noise's, from the Python helper and from the reference
    n = gumbel_noise(SEED, D0, 20, (E, N), DEV).cpu().numpy()
    ref = S.noise(SEED, D0, 20, E * N).reshape(20, E, N, 9)
    assert (n.view(np.uint32) != ref.view(np.uint32)).sum() * 2**20 <= 8 * n.size


def test_set_sampling_none_restores_the_argmax_launch():
    E, N, K = 4, 64, 6
    never, was = FlockVec(E, n_agents=[N], seed=7, device=DEV), FlockVec(E, n_agents=[N], seed=7, device=DEV)
    pol = seeded_policy(4)
    for v in (never, was):
        v.set_policy(pol)
    was.set_sampling(SEED, 5)
    was.set_sampling(None)
    assert was.sampling is None
    act0 = pol.act(never.obs)
    go_a, acts_a, lg_a = tp.launch(never, act0, K, None, True, True)
    go_b, acts_b, lg_b = tp.launch(was, act0, K, None, True, True)
    go_b.assert_equal({f: go_a[f] for f in FKEYS}, "sampling turned off")
    assert torch.equal(acts_a, acts_b) and torch.equal(ibits(lg_a), ibits(lg_b))
    assert_flock_end(never, was, "sampling turned off", outputs=False)
    # and with noise given it is the launch it always was
    noise = tp.noise_rows(K, E, N)
    go_a, acts_a, _ = tp.launch(never, acts_a[K].clone(), K, noise, True, True)
    go_b, acts_b, _ = tp.launch(was, acts_b[K].clone(), K, noise, True, True)
    assert torch.equal(acts_a, acts_b)
    assert_flock_end(never, was, "sampling turned off, noise given", outputs=False)


# ---- 8. refusals that need a world -----------------------------------------------------------------------
def test_refusals():
    E, N, K = 2, 8, 3
    vec = FlockVec(E, n_agents=[N], seed=1, device=DEV)
    w = vec.world
    pol, crit = seeded_policy(4), seeded_critic(4)
    vec.set_policy(pol)
    vec.set_critic(crit)
    vec.set_sampling(SEED, 40)
    act = torch.ones((E, N, 3), dtype=torch.uint8, device=DEV)
    acts = torch.ones((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
    noise = gumbel_noise(SEED, 40, K, (E, N), DEV)
    vals = torch.full((E, N), 7.0, device=DEV)
    tvals = torch.full((K + 1, E, N), 7.0, device=DEV)
    before = vec.get_state()
    # noise given while sampling is on: every entry point, nothing launched, the decision stays
    for call in (lambda: vec.rollout_policy(act, K, noise=noise),
                 lambda: vec.rollout_policy(acts, K, noise=noise, trajectory=True),
                 lambda: vec.rollout_policy(act, K, noise=noise, values=vals),
                 lambda: vec.rollout_policy(acts, K, noise=noise, trajectory=True, values=tvals)):
        with pytest.raises(MacmError, match="sampling is on") as ei:
            call()
        assert ei.value.code == _abi.E_INVALID
    torch.cuda.synchronize()
    assert vec.sampling == (SEED, 40)
    assert bool((act == 1).all()) and bool((acts == 1).all()) and bool((vals == 7.0).all()) and bool((tvals == 7.0).all())
    for k in before:
        np.testing.assert_array_equal(before[k], vec.get_state()[k], err_msg=k)
    # reserved != 0: refused, and the registration stays as it was
    bad = _abi.MacmSampleConfig(1, 2, (ctypes.c_int32 * 4)(0, 0, 1, 0))
    assert w.L.macm_world_set_sampling(w.h, ctypes.byref(bad)) == _abi.E_INVALID
    assert b"reserved" in w.L.macm_last_error() and vec.sampling == (SEED, 40)
    out = _abi.MacmSampleConfig()
    assert w.L.macm_world_get_sampling(w.h, None) == _abi.E_INVALID
    assert w.L.macm_world_get_sampling(w.h, ctypes.byref(out)) == 1 and (out.seed, out.decision) == (SEED, 40)
    # n_steps = 0 does nothing, the decision included
    vec.rollout_policy(act, 0)
    assert vec.sampling == (SEED, 40)
    # a refused launch (no critic registered) does not advance the decision either
    vec.set_critic(None)
    with pytest.raises(MacmError, match="no critic"):
        vec.rollout_policy(act, K, values=vals)
    assert vec.sampling == (SEED, 40)
    vec.rollout_policy(act, K)
    assert vec.sampling == (SEED, 40 + K)
    vec.set_sampling(None)
    assert w.L.macm_world_get_sampling(w.h, ctypes.byref(out)) == 0 and (out.seed, out.decision) == (0, 0)
    # a continuous-action world has no heads to sample
    cont = FlockVec(E, n_agents=[N], seed=1, device=DEV, action_mode="continuous")
    with pytest.raises(MacmError) as ei:
        cont.set_sampling(SEED)
    assert ei.value.code == -4, "MACM_E_UNSUPPORTED for a continuous-action world"
    assert cont.sampling is None
    with pytest.raises(ValueError, match="2\\*\\*64"):
        vec.set_sampling(-1)
