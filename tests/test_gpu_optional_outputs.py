"""`NULL = not wanted` outputs of the C-ABI (include/macm.h: every field of macm_outputs and
macm_tdm_outputs is optional, Flock's reward excepted) and the extent of what the kernels write.

Every other test goes through World._out / TdmWorld._out, which set every field, so the kernels'
`if (obs)`, `if (nbr_out)`, `if (TB.health_out)`, traj_row(p, ...) guards and the host's row / slice
helpers never ran with a NULL field, and nothing checked that a kernel writes only inside the buffers
it is given. Here the entry points are called directly with outputs structs built from a subset of
fields, every buffer the middle of a larger allocation with 256 prefilled bytes on each side
(tests/guard_bands.py). The reference is a twin world, created identically and driven by the same
calls through World / TdmWorld with every field set (the path the rest of the suite pins to the
oracle): after every call the non-NULL fields equal the twin's bit for bit and both bands of every
buffer are intact; at the end state, counters, reward sums, spill count and status are equal. Every
case asserts the launch path it exists for (spill count, launch flags, env slices)."""
import numpy as np
import pytest
import torch

from action_gen import random_flock_actions
from guard_bands import FILL, GuardedOutputs
from parity import assert_state_equal
from test_gpu_tdm import assert_tdm_state_equal
from test_gpu_tdm_split import actions as tdm_actions

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402
from gym_macm.world import World, _ptr  # noqa: E402

DEV = "cuda:0"
FLOCK_SUBSETS = [("reward",), ("reward", "done"), ("reward", "obs"), ("reward", "nbr_id", "collided")]
TDM_SUBSETS = [(), ("done", "winner"), ("obs",), ("mask",), ("health", "alive")]


def ids(subsets):
    return ["+".join(s) or "none" for s in subsets]


def ok(rc, what):
    assert rc == 0, f"{what} returned {rc}: {_abi.lib().macm_last_error().decode()}"


def flock_worlds(E, N, seed, obs_f64=False, debug=0, **kw):
    """(world under test, twin): the same configuration, debug flags and reset."""
    ws = []
    for _ in range(2):
        w = World(to_config(flockSettings(**kw), N, 1, obs_f64=obs_f64), None, E, device=DEV)
        if debug:
            w.set_debug(debug)
        ws.append(w)
    return ws


def flock_actions(K, E, N, seed):
    return random_flock_actions((K, E, N), seed)


def flock_twin_outputs(t):
    return dict(obs=t.obs, nbr_id=t.nbr_id, reward=t.reward, collided=t.collided, done=t.done)


def flock_end(w, t, ctx):
    assert_state_equal(w.get_state(), t.get_state(), ctx)
    np.testing.assert_array_equal(w.counters(), t.counters(), err_msg=f"{ctx}: counters")
    pw, tw = w.reward_sums()
    pt, tt = t.reward_sums()
    np.testing.assert_array_equal(pw, pt, err_msg=f"{ctx}: reward sums")
    assert tw == tt and w.spilled() == t.spilled(), ctx
    assert w.status() == 0 and t.status() == 0, ctx


def flock_drive(w, t, subset, seed, n_step, K, forms):
    """reset (NULL or the subset's obs / nbr_id), then the forms, each compared with the twin."""
    E, N = w.E, w.N
    L, s = w.L, w._stream()
    init = tuple(f for f in subset if f in ("obs", "nbr_id"))
    o = GuardedOutputs(w, init)
    ok(L.macm_world_reset(w.h, seed, 0, o.ref() if init else None, s), "reset")
    t.reset(seed, 0)
    o.assert_equal(flock_twin_outputs(t), "reset")
    acts = flock_actions(n_step + 2 * K, E, N, seed)
    o = GuardedOutputs(w, subset)
    if "step" in forms:
        for k in range(n_step):
            ok(L.macm_world_step(w.h, _ptr(acts[k]), o.ref(), s), "step")
            t.step(acts[k])
            o.assert_equal(flock_twin_outputs(t), f"step {k}")
    if "rollout" in forms:  # the carried steps of the wave kernel; the workgroup path's launches per step
        a = acts[n_step:n_step + K]
        ok(L.macm_world_rollout(w.h, _ptr(a), K, o.ref(), s), "rollout")
        t.rollout(a)
        o.assert_equal(flock_twin_outputs(t), "rollout")
    if "traj" in forms:
        a = acts[n_step + K:]
        ot = GuardedOutputs(w, subset, n_steps=K)
        ok(L.macm_world_rollout_traj(w.h, _ptr(a), K, ot.ref(), s), "rollout_traj")
        ot.assert_equal(t.rollout_traj(a), "rollout_traj")
    if "observe" in forms:
        oo = GuardedOutputs(w, init)
        ok(L.macm_world_observe(w.h, oo.ref(), s), "observe")
        t.observe()
        oo.assert_equal(flock_twin_outputs(t), "observe")
    o.check_bands("end")
    flock_end(w, t, "end")


ALL_FORMS = ("step", "rollout", "traj", "observe")


@pytest.mark.parametrize("subset", FLOCK_SUBSETS, ids=ids(FLOCK_SUBSETS))
@pytest.mark.parametrize("N,obs_f64", [(20, False), (20, True), (64, False), (64, True)])
def test_flock_wave_partial_outputs(N, obs_f64, subset):
    """The wave kernel (flock_step_w64.hip: `if (coll_out)`, `if (nbr_out)`, `if (obs)`, `if (done_out)`
    of the step, traj_row of the rollout's rows) in its 32-lane (N = 20) and 64-lane instantiations, both
    obs widths: per-step launches, the rollout's carried steps, the trajectory rows and observe. Lanes
    >= N of the last env must not store (the band behind every buffer)."""
    w, t = flock_worlds(4, N, 11 + N, obs_f64)
    flock_drive(w, t, subset, 11 + N, 3, 3, ALL_FORMS)
    assert w.N <= 64 and w.spilled() == 0 and w.launch_flags() == 0 and w.rollout_slices() == 0, \
        "not the wave kernel's fast step"


@pytest.mark.parametrize("subset", FLOCK_SUBSETS, ids=ids(FLOCK_SUBSETS))
def test_flock_wave_spill_partial_outputs(subset):
    """The spill step called from the wave kernel (flock_spill.hpp step_env: `if (coll_out)`,
    `if (nbr_out)`, `if (obs)`, `if (done_out)`), every env sent there by MACM_DEBUG_FORCE_SPILL."""
    w, t = flock_worlds(4, 64, 5, debug=_abi.DEBUG_FORCE_SPILL, start_spread=8)
    flock_drive(w, t, subset, 5, 3, 3, ALL_FORMS)
    assert w.spilled() == 4 * (3 + 3 + 3), "the envs did not take the spill step"


@pytest.mark.parametrize("debug", [0, _abi.DEBUG_FORCE_SPILL], ids=["fast", "spill"])
@pytest.mark.parametrize("subset", FLOCK_SUBSETS, ids=ids(FLOCK_SUBSETS))
def test_flock_workgroup_partial_outputs(subset, debug):
    """The workgroup path (flock_step_wg.hip kernel C's guards; capi_world.hip step_outputs' rows of the
    trajectory form) at N = 100: a block of 128 threads, 28 of them without a body in every env. Once
    with every env in the spill step (kernel A's call of flock_spill.hpp step_env)."""
    E = 3
    w, t = flock_worlds(E, 100, 17, debug=debug)
    flock_drive(w, t, subset, 17, 3, 3, ("step", "rollout", "traj", "observe"))
    assert 64 < w.N <= 1024 and w.rollout_slices() == 0
    assert w.spilled() == (E * 9 if debug else 0), "not the path this case exists for"
    assert w.launch_flags() == t.launch_flags()


@pytest.mark.parametrize("subset", [("reward",), ("reward", "done")], ids=["reward", "reward+done"])
def test_flock_sliced_rollout_partial_outputs(subset):
    """The workgroup path's rollout in env slices on streams of their own (capi_world.hip
    rollout_wg_slices: `row(p, per_env)` keeps a NULL field NULL for every slice, step_outputs for every
    step), 1031 envs: uneven slices."""
    E, N, K = 1031, 100, 4
    w, t = flock_worlds(E, N, 8, start_spread=12)
    flock_drive(w, t, subset, 8, 0, K, ("rollout", "traj"))
    assert w.rollout_slices() >= 2, "the rollout did not run in env slices"


@pytest.mark.parametrize("subset", FLOCK_SUBSETS, ids=ids(FLOCK_SUBSETS))
def test_flock_big_partial_outputs(subset):
    """The big path (flock_big.hip: the init and observe kernels' `if (nbr_out)` / `if (obs)`, and
    flock_spill.hpp step_env with 2 bodies per thread) at N = 1025: the second pass holds one body."""
    w, t = flock_worlds(1, 1025, 3, start_spread=30)
    flock_drive(w, t, subset, 3, 2, 2, ("step", "traj", "observe"))
    assert w.spilled() == 4, "N > 1024 steps every env with the spill step"


# ---- TDM -------------------------------------------------------------------------------------------

FORMS = {
    "default": {},  # the world's choice: below 1024 envs the split step / rollout and the tail trajectory
    "fused": {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "0"},
    "split": {"MACM_TDM_SPLIT_OBS": "1", "MACM_TDM_TAIL_OBS": "0"},  # the trajectory in split chunks
}


def tdm_worlds(E, teams, seed, **kw):
    return [TdmWorld(tdm_config(teams, **kw), E, device=DEV) for _ in range(2)]


def tdm_twin_outputs(t):
    return dict(zip(TdmWorld._TRAJ_KEYS, t.outputs()))


def tdm_end(w, t, ctx):
    assert_tdm_state_equal(w.get_state(), t.get_state(), ctx)
    np.testing.assert_array_equal(w.counters(), t.counters(), err_msg=f"{ctx}: counters")
    assert w.spilled() == t.spilled(), ctx
    assert w.status() == 0 and t.status() == 0, ctx


def tdm_drive(w, t, subset, seed, n_step, K, forms):
    E, N = w.E, w.N
    L, s = w.L, w._stream()
    o = GuardedOutputs(w, subset)
    ok(L.macm_tdm_reset(w.h, seed, 0, o.ref() if subset else None, s), "reset")
    t.reset(seed, 0)
    o.assert_equal(tdm_twin_outputs(t), "reset")
    acts = tdm_actions(n_step + 2 * K, E, N, seed)
    for k in range(n_step):
        ok(L.macm_tdm_step(w.h, _ptr(acts[k]), o.ref() if subset else None, s), "step")  # none: out = NULL
        t.step(acts[k])
        o.assert_equal(tdm_twin_outputs(t), f"step {k}")
    if "rollout" in forms:
        a = acts[n_step:n_step + K]
        ok(L.macm_tdm_rollout(w.h, _ptr(a), K, o.ref() if subset else None, s), "rollout")
        t.rollout(a)
        o.assert_equal(tdm_twin_outputs(t), "rollout")
    if "traj" in forms:
        a = acts[n_step + K:]
        ot = GuardedOutputs(w, subset, n_steps=K)
        ok(L.macm_tdm_rollout_traj(w.h, _ptr(a), K, ot.ref(), s), "rollout_traj")  # none: every field NULL
        ot.assert_equal(t.rollout_traj(a), "rollout_traj")
    oo = GuardedOutputs(w, subset)
    ok(L.macm_tdm_observe(w.h, oo.ref(), s), "observe")
    t.observe()
    oo.assert_equal(tdm_twin_outputs(t), "observe")
    o.check_bands("end")
    tdm_end(w, t, "end")


@pytest.mark.parametrize("subset", TDM_SUBSETS, ids=ids(TDM_SUBSETS))
@pytest.mark.parametrize("form", list(FORMS))
def test_tdm_wave_partial_outputs(monkeypatch, form, subset):
    """The TDM wave kernel (flock_step_w64.hip: `if (TB.health_out)`, `if (TB.alive_out)`,
    `if (TB.winner_out)`, `if (done_out)`, the rollout's traj_row; tdm_obs.hpp: `if (obs)` / `if (mask)`
    of every store) with the observation fused into the step, split off (tdm_obs_snap.hip: `o` / `m`
    NULL; capi_tdm.hip tdm_rollout_split's row()) and in the launch's tail (tdm_tail_row's obs_r /
    mask_r), at [8, 8]. obs without mask and mask without obs take the observation path with one of the
    two NULL; the subsets without either must skip it."""
    E, teams, K = 4, [8, 8], 5
    for k in ("MACM_TDM_SPLIT_OBS", "MACM_TDM_TAIL_OBS", "MACM_TDM_TAIL_WORKERS", "MACM_TDM_TAIL_STEPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    w, t = tdm_worlds(E, teams, 21, world_width=10.0, world_height=10.0)
    flags = w.launch_flags()
    if form == "fused":
        assert flags == 0, flags
    elif form == "split":
        assert flags & _abi.LAUNCH_SPLIT_OBS and not flags & _abi.LAUNCH_TAIL_OBS, flags
    else:  # the world's own choice at 4 envs
        assert flags & _abi.LAUNCH_SPLIT_OBS and flags & _abi.LAUNCH_TAIL_OBS, flags
    tdm_drive(w, t, subset, 21, 2, K, ("rollout", "traj"))
    assert int(w.counters()[1]) > 0, "no melee attack: the casts and health stores did not run"
    assert w.spilled() == 0, "not the wave kernel's fast step"


@pytest.mark.parametrize("subset", TDM_SUBSETS, ids=ids(TDM_SUBSETS))
def test_tdm_workgroup_partial_outputs(subset):
    """The workgroup TDM step (tdm_step_wg.hip: `if (TB.health_out)`, `if (TB.alive_out)`,
    `if (TB.winner_out)`; flock_spill.hpp step_env's TDM env layer and tdm_obs_block; capi_tdm.hip
    tdm_rollout's row() per step) at [33, 32]: 65 agents on a block of 128 threads."""
    E = 2
    w, t = tdm_worlds(E, [33, 32], 9, world_width=14.0, world_height=14.0)
    tdm_drive(w, t, subset, 9, 2, 3, ("traj",))
    assert w.spilled() == E * 5, "every env-step above 64 agents is the workgroup step's"


@pytest.mark.parametrize("subset", TDM_SUBSETS, ids=ids(TDM_SUBSETS))
def test_tdm_two_bodies_per_thread_partial_outputs(subset):
    """The workgroup TDM step with two bodies per thread ([513, 512]: tdm_obs_block_linear's
    `if (obs)` / `if (mask)` over 1025 x 1024 slots, the last thread's lone second body)."""
    w, t = tdm_worlds(1, [513, 512], 4, world_width=60.0, world_height=60.0)
    tdm_drive(w, t, subset, 4, 2, 0, ())
    assert w.spilled() == 2


# ---- reset, place, reset_envs ------------------------------------------------------------------------


def fill_twin(t, names):
    for f in names:
        getattr(t, f).view(torch.uint8).fill_(FILL)


@pytest.mark.parametrize("init", [(), ("obs",), ("nbr_id",), ("obs", "nbr_id")], ids=["none", "obs", "nbr_id", "both"])
@pytest.mark.parametrize("E,N,spread", [(5, 20, 20.0), (5, 100, 20.0), (2, 1025, 30.0)])
def test_flock_reset_place_reset_envs_partial_outputs(E, N, spread, init):
    """macm_world_reset / place / reset_envs with out = NULL and a partial out (the init kernels of the
    wave, workgroup and big paths: `if (nbr_out)`, `if (obs)`). reset_envs with a mask writes the reset
    envs' rows only: the other envs' rows keep the prefill, in every buffer."""
    w, t = flock_worlds(E, N, 2, start_spread=spread)
    L, s = w.L, w._stream()
    o = GuardedOutputs(w, init)
    ok(L.macm_world_reset(w.h, 40, 7, o.ref() if init else None, s), "reset")
    t.reset(40, 7)
    o.assert_equal(flock_twin_outputs(t), "reset")
    a = flock_actions(2, E, N, 1)
    full = GuardedOutputs(w, ("reward",))
    for k in range(2):
        ok(L.macm_world_step(w.h, _ptr(a[k]), full.ref(), s), "step")
        t.step(a[k])
    mask = np.arange(E) % 2 == 0  # envs 0, 2, 4 (E = 2: env 0)
    dm = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    o = GuardedOutputs(w, init)  # fresh: every row holds the prefill
    fill_twin(t, ("obs", "nbr_id"))
    ok(L.macm_world_reset_envs(w.h, _ptr(dm), o.ref() if init else None, s), "reset_envs")
    t.reset_envs(dm)
    o.assert_equal(flock_twin_outputs(t), "reset_envs")  # the reset envs' rows, and the prefill of the others
    for f in init:
        assert o.bufs[f].rows_untouched(~mask), f"reset_envs wrote {f} rows of envs it did not reset"
        assert not o.bufs[f].rows_untouched(mask), f"reset_envs did not write the reset envs' {f} rows"
    assert_state_equal(w.get_state(), t.get_state(), "reset_envs")
    ok(L.macm_world_reset_envs(w.h, None, None, s), "reset_envs(all, NULL)")
    t.reset_envs()
    assert_state_equal(w.get_state(), t.get_state(), "reset_envs of all envs")
    st = t.get_state()
    pos, ang, tg = st["pos"][::-1].copy(), st["angle"][::-1].copy(), st["targets"].copy()
    o = GuardedOutputs(w, init)
    ok(L.macm_world_place(w.h, pos.ctypes.data, ang.ctypes.data, tg.ctypes.data, o.ref() if init else None, s), "place")
    t.place(pos, ang, tg)
    o.assert_equal(flock_twin_outputs(t), "place")
    flock_end(w, t, "place")


@pytest.mark.parametrize("subset", [(), ("obs",), ("mask", "winner"), ("health", "alive", "done")],
                         ids=["none", "obs", "mask+winner", "health+alive+done"])
@pytest.mark.parametrize("E,teams", [(5, [8, 8]), (3, [33, 32])])
def test_tdm_reset_place_reset_envs_partial_outputs(E, teams, subset):
    """macm_tdm_reset / place / reset_envs with out = NULL and a partial out (tdm_init_w64 and the
    workgroup init kernel: `if (TB.health_out)`, `if (TB.alive_out)`, `if (TB.winner_out)`, the obs /
    mask pointers; the host's `if (out && out->done)`). reset_envs with a mask leaves the other envs'
    rows untouched."""
    w, t = tdm_worlds(E, teams, 6, world_width=12.0, world_height=12.0)
    L, s = w.L, w._stream()
    N = w.N
    o = GuardedOutputs(w, subset)
    ok(L.macm_tdm_reset(w.h, 6, 3, o.ref() if subset else None, s), "reset")
    t.reset(6, 3)
    o.assert_equal(tdm_twin_outputs(t), "reset")
    a = tdm_actions(2, E, N, 5)
    for k in range(2):
        ok(L.macm_tdm_step(w.h, _ptr(a[k]), None, s), "step")
        t.step(a[k])
    mask = np.arange(E) % 2 == 1
    dm = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    o = GuardedOutputs(w, subset)
    fill_twin(t, TdmWorld._TRAJ_KEYS)
    ok(L.macm_tdm_reset_envs(w.h, _ptr(dm), o.ref() if subset else None, s), "reset_envs")
    t.reset_envs(dm)
    o.assert_equal(tdm_twin_outputs(t), "reset_envs")
    for f in subset:
        assert o.bufs[f].rows_untouched(~mask), f"reset_envs wrote {f} rows of envs it did not reset"
        if f != "done":  # the new episodes' done flags are the state's; the output is not written
            assert not o.bufs[f].rows_untouched(mask), f"reset_envs did not write the reset envs' {f} rows"
    assert_tdm_state_equal(w.get_state(), t.get_state(), "reset_envs")
    ok(L.macm_tdm_reset_envs(w.h, None, None, s), "reset_envs(all, NULL)")
    t.reset_envs()
    assert_tdm_state_equal(w.get_state(), t.get_state(), "reset_envs of all envs")
    st = t.get_state()
    pos, ang = st["pos"][::-1].copy(), st["angle"][::-1].copy()
    o = GuardedOutputs(w, subset)
    ok(L.macm_tdm_place(w.h, pos.ctypes.data, ang.ctypes.data, o.ref() if subset else None, s), "place")
    t.place(pos, ang)
    o.assert_equal(tdm_twin_outputs(t), "place")
    tdm_end(w, t, "place")


# ---- host refusals -----------------------------------------------------------------------------------


def test_flock_required_outputs_are_refused_on_the_host():
    """Flock's reward is required by step and every rollout form, obs by the closed loop (the bots act
    on it): MACM_E_INVALID from the host checks (capi_world.hip macm_world_step, world_rollout), nothing
    launched: state, step counts and counters as before, every buffer untouched."""
    E, N, K = 3, 20, 2
    w, _ = flock_worlds(E, N, 1)
    w.reset(4, 0)
    L, s = w.L, w._stream()
    a = flock_actions(K + 1, E, N, 2)
    before, c0 = w.get_state(), w.counters()
    no_reward = GuardedOutputs(w, ("obs", "nbr_id", "collided", "done"))
    no_reward_k = GuardedOutputs(w, ("obs", "nbr_id", "collided", "done"), n_steps=K)
    no_obs = GuardedOutputs(w, ("reward", "nbr_id"))
    no_obs_k = GuardedOutputs(w, ("reward", "nbr_id"), n_steps=K)
    calls = [
        L.macm_world_step(w.h, _ptr(a[0]), no_reward.ref(), s),
        L.macm_world_step(w.h, _ptr(a[0]), None, s),
        L.macm_world_rollout(w.h, _ptr(a), K, no_reward.ref(), s),
        L.macm_world_rollout_traj(w.h, _ptr(a), K, no_reward_k.ref(), s),
        L.macm_world_rollout_bots(w.h, _ptr(a[0]), K, no_obs.ref(), s),
        L.macm_world_rollout_bots_traj(w.h, _ptr(a), K, no_obs_k.ref(), s),
        L.macm_world_rollout_bots(w.h, _ptr(a[0]), K, no_reward.ref(), s),
    ]
    assert calls == [_abi.E_INVALID] * len(calls), calls
    torch.cuda.synchronize()
    for o in (no_reward, no_reward_k, no_obs, no_obs_k):
        o.check_bands("refused call")
        for f, g in o.bufs.items():
            assert g.rows_untouched(np.ones(g.t.shape[0], bool)), f"a refused call wrote {f}"
    assert_state_equal(w.get_state(), before, "after the refused calls")
    np.testing.assert_array_equal(w.counters(), c0)
    assert (w.get_state()["step_count"] == 0).all() and w.status() == 0


@pytest.mark.parametrize("teams", [[8, 8], [33, 32]])
def test_tdm_closed_loop_needs_obs_and_mask(teams):
    """macm_tdm_rollout_bots / _traj with obs or mask NULL (the bots read both inside the launch; the
    wave kernel would offset a NULL mask): MACM_E_INVALID from tdm_rollout's host check, nothing launched."""
    E, K = 2, 2
    w, _ = tdm_worlds(E, teams, 1)
    w.reset(4, 0)
    L, s = w.L, w._stream()
    N = w.N
    a = tdm_actions(K + 1, E, N, 2)
    before, c0 = w.get_state(), w.counters()
    outs, calls = [], []
    for fields in (("obs", "health"), ("mask", "done"), ("winner",)):
        o, ok_ = GuardedOutputs(w, fields), GuardedOutputs(w, fields, n_steps=K)
        outs += [o, ok_]
        calls.append(L.macm_tdm_rollout_bots(w.h, _ptr(a[0]), K, o.ref(), s))
        calls.append(L.macm_tdm_rollout_bots_traj(w.h, _ptr(a), K, ok_.ref(), s))
    calls.append(L.macm_tdm_rollout_bots(w.h, _ptr(a[0]), K, None, s))
    assert calls == [_abi.E_INVALID] * len(calls), calls
    torch.cuda.synchronize()
    for o in outs:
        o.check_bands("refused call")
        for f, g in o.bufs.items():
            assert g.rows_untouched(np.ones(g.t.shape[0], bool)), f"a refused call wrote {f}"
    assert_tdm_state_equal(w.get_state(), before, "after the refused calls")
    np.testing.assert_array_equal(w.counters(), c0)
    assert (w.get_state()["step_count"] == 0).all() and w.status() == 0

