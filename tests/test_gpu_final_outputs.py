"""Final outputs of an autoreset world (macm_world_set_final_outputs / macm_tdm_set_final_outputs): the
obs / nbr_id (TDM: obs / mask) that the reset overwrites in the output row of a step that sets done, the
ended episode's length and a count of the ends, kept per env.

The bar is the twin of test_gpu_rollout_autoreset.py: a world with the same seed and autoreset off,
driven by the loop `step -> capture obs / nbr_id / mask and step_count -> reset_envs(done)`. The final
row of env e is the capture at the last step that set done[e], bit for bit (the same kernels' stores,
copied); length is the captured step count; ends the number of such steps. The final buffers are
guarded allocations prefilled with FILL: rows of envs that did not end still hold it, and so do the
bands. Every case also checks that the trajectory and the end state are still the loop's: registering
the buffers changes nothing else."""
import ctypes

import numpy as np
import pytest
import torch

from guard_bands import FILL, Guarded, GuardedOutputs
from test_gpu_parity import obs_check
from test_gpu_rollout import flock_actions
from test_gpu_rollout_autoreset import (FKEYS, TKEYS, assert_flock_end, flock_twins, tdm_random_actions, tdm_twins)
from test_gpu_trajectory import assert_tdm_state, assert_traj

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm._abi import MacmError  # noqa: E402
from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.bots import flock_actions as bot_flock  # noqa: E402
from gym_macm.settings import flockSettings, to_config  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402
from parity import oracle_for  # noqa: E402

DEV = "cuda:0"
F64C = {"obs_dtype": torch.float64, "coord": "cartesian"}


def bits(t):
    return t.contiguous().view(torch.uint8)


# ---- guarded final buffers ---------------------------------------------------------------------------
class FinalBufs:
    """A guarded buffer for every final field of world `w`'s kind; those in `fields` (default: all) go
    into the macm_final_outputs registered with the world, the others stay NULL there. ends is zeroed
    when it is set, as the caller must; everything else starts as FILL."""

    def __init__(self, w, fields=None, register=True, zero_ends=True):
        self.tdm = isinstance(w, TdmWorld)
        odt = torch.float64 if w.cfg.obs_f64 else torch.float32
        E, N = w.E, w.N
        if self.tdm:
            spec = dict(obs=(odt, (E, N, N - 1, 4)), mask=(torch.uint8, (E, N, N - 1)))
        else:
            spec = dict(obs=(odt, (E, N, w.OD)), nbr_id=(torch.int32, (E, N)))
        spec.update(length=(torch.int32, (E,)), ends=(torch.int32, (E,)))
        self.g = {f: Guarded(shp, dt, w.device) for f, (dt, shp) in spec.items()}
        self.set = tuple(spec) if fields is None else tuple(fields)
        assert set(self.set) <= set(spec)
        self.zero_ends = zero_ends and "ends" in self.set
        if self.zero_ends:
            self.g["ends"].t.zero_()
        self.struct = _abi.MacmFinalOutputs(**{f: ctypes.c_void_p(self.g[f].t.data_ptr()) for f in self.set})
        self.E = E
        if register:
            w._register_final(self.struct)

    def __getitem__(self, f):
        return self.g[f].t

    def all_fill(self, skip=()):
        torch.cuda.synchronize()
        return all(bool((g.raw == FILL).all()) for f, g in self.g.items() if f not in skip)

    def same_bytes(self, other):
        torch.cuda.synchronize()
        return all(torch.equal(self.g[f].bytes, other.g[f].bytes) for f in self.g)

    def check(self, cap, ctx):
        """The set fields hold the capture's rows for the envs that ended and FILL elsewhere; the fields
        that are not set hold FILL; no band was written."""
        torch.cuda.synchronize()
        all_rows = np.ones(self.E, bool)
        ended = torch.as_tensor(cap.ended, device=DEV)
        for f, g in self.g.items():
            assert g.bands_intact(), f"{ctx}: a store outside the final {f} buffer"
            if f not in self.set:
                assert g.rows_untouched(all_rows), f"{ctx}: final {f} is not registered but was written"
            elif f == "ends":
                assert self.zero_ends
                np.testing.assert_array_equal(g.t.cpu().numpy(), cap.ends, err_msg=f"{ctx}: ends")
            else:
                assert g.rows_untouched(~cap.ended), f"{ctx}: final {f} row of an env that did not end was written"
                if not cap.ended.any():
                    continue
                if f == "length":
                    np.testing.assert_array_equal(g.t.cpu().numpy()[cap.ended], cap.length[cap.ended],
                                                  err_msg=f"{ctx}: length")
                else:
                    assert torch.equal(bits(g.t[ended]), bits(cap.rows[f][ended])), \
                        f"{ctx}: final {f} differs from what the ending step wrote with autoreset off"


class Capture:
    """What the loop's world shows between a step that set done and the reset that follows."""

    def __init__(self, E):
        self.rows = {}
        self.length = np.zeros(E, np.int32)
        self.ends = np.zeros(E, np.int32)
        self.ended = np.zeros(E, bool)
        self.at = []  # (step index, env) of every end, in order

    def take(self, k, done, fields, world):
        if not bool(done.any()):
            return
        d = done.bool()
        for f, t in fields.items():
            if f not in self.rows:
                self.rows[f] = torch.zeros_like(t)
            self.rows[f][d] = t[d]
        dn = d.cpu().numpy()
        self.length[dn] = world.get_state()["step_count"][dn]
        self.ends[dn] += 1
        self.ended |= dn
        self.at += [(k, int(e)) for e in np.flatnonzero(dn)]


# ---- the loop of test_gpu_rollout_autoreset.py, capturing before each reset ------------------------------
def flock_step_cap(vec, act, cap, k):
    w = vec.world
    w.step(act)
    row = {f: getattr(w, f).clone() for f in ("reward", "collided", "done")}
    cap.take(k, row["done"], dict(obs=w.obs, nbr_id=w.nbr_id), w)
    w.reset_envs(row["done"].clone())
    row["obs"], row["nbr_id"] = w.obs.clone(), w.nbr_id.clone()
    return row


def flock_loop_cap(vec, acts, cap):
    rows = [flock_step_cap(vec, acts[k], cap, k) for k in range(acts.shape[0])]
    return {f: torch.stack([r[f] for r in rows]) for f in FKEYS}


def flock_loop_bots_cap(vec, act, K, cap):
    act = act.clone()
    rows, arows = [], [act.clone()]
    for k in range(K):
        rows.append(flock_step_cap(vec, act, cap, k))
        bot_flock(vec.world.obs, out=act)
        arows.append(act.clone())
    return {f: torch.stack([r[f] for r in rows]) for f in FKEYS}, torch.stack(arows)


def tdm_step_cap(w, act, cap, k):
    w.step(act)
    row = {f: getattr(w, f).clone() for f in ("health", "alive", "done", "winner")}
    cap.take(k, row["done"], dict(obs=w.obs, mask=w.mask), w)
    w.reset_envs(row["done"].clone())
    row["obs"], row["mask"] = w.obs.clone(), w.mask.clone()
    return row


def tdm_loop_cap(w, acts, cap):
    rows = [tdm_step_cap(w, acts[k], cap, k) for k in range(acts.shape[0])]
    return {f: torch.stack([r[f] for r in rows]) for f in TKEYS}


def tdm_loop_bots_cap(w, act, K, cap, k0=0):
    act = act.clone()
    rows, arows = [], [act.clone()]
    for k in range(K):
        rows.append(tdm_step_cap(w, act, cap, k0 + k))
        combat_actions(w.obs, w.mask, out=act)
        arows.append(act.clone())
    return {f: torch.stack([r[f] for r in rows]) for f in TKEYS}, torch.stack(arows)


def two_phase_start(off, on, E, N):
    """5 steps, then reset_envs on the odd envs (test_flock_64_two_phases_in_one_launch): with
    time_limit = 0.25 at 60 Hz an episode ends at its 16th step, so the even envs end at rows 10 and 26
    of what follows and the odd envs at rows 15 and 31."""
    pre = flock_actions(5, E, N, 3)
    for k in range(5):
        off.step(pre[k])
        on.step(pre[k])
    half = torch.tensor([e % 2 for e in range(E)], dtype=torch.uint8, device=DEV)
    off.reset_envs(half)
    on.reset_envs(half)
    return pre, half


# ---- 1. Flock wave path: two ends of every env in one launch, against the loop and the oracle -----------
@pytest.mark.parametrize("reload", [0, 1])
@pytest.mark.parametrize("kw", [{}, F64C], ids=["f32polar", "f64cart"])
def test_flock_wave_two_ends_in_one_launch(kw, reload):
    E, N, K, seed = 8, 64, 40, 5
    off, on = flock_twins(E, N, seed, time_limit=0.25, **kw)
    if reload:
        on.world.set_debug(_abi.DEBUG_ROLLOUT_RELOAD)
    fin = FinalBufs(on.world)
    pre, half = two_phase_start(off, on, E, N)
    assert fin.all_fill(skip=("ends",)) and int(fin["ends"].sum()) == 0, "steps without an end, reset_envs: no write"
    acts = flock_actions(K, E, N, 11)
    cap = Capture(E)
    ref = flock_loop_cap(off, acts, cap)
    traj = on.rollout(acts, trajectory=True)
    assert_traj(ref, traj, "trajectory")
    done = traj["done"].cpu().numpy()
    assert [list(np.flatnonzero(done[:, e])) for e in (0, 1)] == [[10, 26], [15, 31]]
    fin.check(cap, "two ends")
    assert (cap.ends == 2).all() and (cap.length == 16).all()
    assert_flock_end(off, on, "after the rollout")
    # the oracle through the same calls: its obs at the last step that set done (ids exact, obs by the
    # rule for the world's obs dtype)
    okw = {k: v for k, v in kw.items() if k != "obs_dtype"}
    orc = oracle_for(to_config(flockSettings(time_limit=0.25, **okw), N, 1, obs_f64=True), None, E, seed)
    for a in pre.cpu().numpy():
        assert not orc.step(a)["done"].any()
    orc.reset_envs(half.cpu().numpy())
    o_obs, o_nbr = None, None
    for a in acts.cpu().numpy():
        r = orc.step(a)
        d = r["done"].astype(bool)
        if d.any():
            if o_obs is None:
                o_obs, o_nbr = np.zeros_like(r["obs"]), np.zeros_like(r["nbr_id"])
            o_obs[d], o_nbr[d] = r["obs"][d], r["nbr_id"][d]
            orc.reset_envs(r["done"])
    np.testing.assert_array_equal(fin["nbr_id"].cpu().numpy(), o_nbr, err_msg="final nbr_id vs oracle")
    obs_check(fin["obs"].cpu().numpy(), o_obs, "obs_dtype" in kw, "final obs vs oracle")


# ---- 2. some envs end, some do not --------------------------------------------------------------------
def test_flock_rows_of_envs_that_did_not_end_are_untouched():
    E, N, K = 8, 64, 12
    off, on = flock_twins(E, N, 5, time_limit=0.25)
    fin = FinalBufs(on.world)
    two_phase_start(off, on, E, N)
    acts = flock_actions(K, E, N, 11)
    cap = Capture(E)
    ref = flock_loop_cap(off, acts, cap)
    assert_traj(ref, on.rollout(acts, trajectory=True), "trajectory")
    # from the time limit alone: the even envs are at their 16th step in row 10, the odd envs at their 12th in row 11
    even = np.arange(E) % 2 == 0
    np.testing.assert_array_equal(cap.ended, even)
    fin.check(cap, "K = 12")
    for f in ("obs", "nbr_id", "length"):
        assert fin.g[f].rows_untouched(~even), f
    np.testing.assert_array_equal(fin["ends"].cpu().numpy(), even.astype(np.int32))
    assert_flock_end(off, on, "K = 12")


# ---- 3. Flock instantiations --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,kw", [
    (32, 56, {}),
    (32, 56, {"obs_dtype": torch.float64}),
    (3, 40, {}),
    (32, 40, {"action_mode": "continuous"}),
    (64, 20, {"action_mode": "continuous"}),
])
def test_flock_instantiations(N, K, kw):
    E, seed = 4, 9
    off, on = flock_twins(E, N, seed, time_limit=0.25, **kw)
    fin = FinalBufs(on.world)
    acts = flock_actions(K, E, N, 21, kw.get("action_mode") == "continuous")
    cap = Capture(E)
    assert_traj(flock_loop_cap(off, acts, cap), on.rollout(acts, trajectory=True), f"N = {N} {kw}")
    assert (cap.ends == K // 16).all() and (cap.length == 16).all()
    fin.check(cap, f"N = {N} {kw}")
    assert_flock_end(off, on, f"N = {N} {kw}")


# ---- 4. every form leaves the final rows of the trajectory launch --------------------------------------
@pytest.mark.parametrize("form,N,K", [("overwrite", 64, 16), ("overwrite", 20, 16), ("steps", 64, 16),
                                      ("bots", 64, 40), ("bots_traj", 64, 40)])
def test_flock_forms_agree_with_the_trajectory_launch(form, N, K):
    E, seed = 8, 17
    bots = form.startswith("bots")
    kw = F64C if bots else {}
    off, a = flock_twins(E, N, seed, time_limit=0.25, **kw)
    b = FlockVec(E, n_agents=[N], seed=seed, device=DEV, autoreset=True, time_limit=0.25, **kw)
    fa, fb = FinalBufs(a.world), FinalBufs(b.world)
    cap = Capture(E)
    if bots:
        act0 = bot_flock(off.obs)
        ref, arows = flock_loop_bots_cap(off, act0, K, cap)
        acts = arows[:K].contiguous()  # the actions the closed loop took
    else:
        acts = flock_actions(K, E, N, 41)
        ref = flock_loop_cap(off, acts, cap)
    assert_traj(ref, a.rollout(acts, trajectory=True), "trajectory launch")
    fa.check(cap, "trajectory launch")
    if form == "overwrite":
        obs, nbr, rew, done = b.rollout(acts)
        assert bool(done.all()), "every env ends in the launch's last step"
        assert torch.equal(obs, ref["obs"][K - 1]) and torch.equal(nbr, ref["nbr_id"][K - 1])
        assert not torch.equal(bits(fb["obs"]), bits(obs)), "the final obs is not the new episode's"
    elif form == "steps":
        for k in range(K):
            obs, nbr, rew, done = b.step(acts[k])
            for f, t in zip(("obs", "nbr_id", "reward", "done"), (obs, nbr, rew, done)):
                assert torch.equal(t, ref[f][k]), f"step {k}: {f}"
    elif form == "bots":
        act = act0.clone()
        b.rollout_bots(act, K)
        assert torch.equal(act, arows[K])
    else:
        buf = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        buf[0] = act0
        assert_traj(ref, b.rollout_bots(buf, K, trajectory=True), "closed-loop trajectory")
        assert torch.equal(buf, arows)
    fb.check(cap, form)
    assert fa.same_bytes(fb), f"{form}: final buffers differ from the trajectory launch's"
    assert (cap.ends == K // 16).all() and (cap.length == 16).all()
    assert_flock_end(off, b, form)
    assert_flock_end(off, a, "trajectory launch")


# ---- 5. TDM wave path ----------------------------------------------------------------------------------
def fused_observation(monkeypatch):
    """The loop's steps observe inside the step kernel, as every step of an autoreset rollout does, so
    that the same writer is compared with itself. (When this was written the step kernel's row-block stage
    wrote -0.0 into the p of a masked slot, a dead agent's, where the split observation, step()'s default
    below 1024 envs, wrote +0.0; the stage has since been corrected and tests/test_gpu_tdm_obs_bits.py
    holds every writer to the same bits.)"""
    monkeypatch.setenv("MACM_TDM_SPLIT_OBS", "0")


@pytest.mark.parametrize("teams,bots,obs_f64", [([32, 32], False, False), ([32, 32], True, False),
                                                ([16, 16], True, True), ([10, 10], False, False)])
def test_tdm_time_limit_ends(teams, bots, obs_f64, monkeypatch):
    fused_observation(monkeypatch)
    E, K, N = 4, 20, sum(teams)
    off, on = tdm_twins(teams, E, 7, obs_f64=obs_f64, time_limit=0.25)
    fin = FinalBufs(on)
    if N == 20:
        assert (N * (N - 1)) % 16 != 0  # an env's mask row does not start 16-byte aligned
    cap = Capture(E)
    if bots:
        act0 = combat_actions(off.obs, off.mask)
        ref, arows = tdm_loop_bots_cap(off, act0, K, cap)
        acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
        acts[0] = act0
        traj = on.rollout_bots_traj(acts, K)
        assert torch.equal(acts, arows)
    else:
        acts = tdm_random_actions(K, E, N, 5)
        ref = tdm_loop_cap(off, acts, cap)
        traj = on.rollout_traj(acts)
    assert_traj(ref, traj, f"TDM {teams}")
    assert bool(traj["done"][15].all()) and int(traj["done"].sum()) == E
    assert (cap.ends == 1).all() and (cap.length == 16).all()
    fin.check(cap, f"TDM {teams}")
    assert_tdm_state(off, on)


def test_tdm_combat_ends_accumulate_over_launches(monkeypatch):
    fused_observation(monkeypatch)
    E, teams, seed, K, launches = 16, [4, 4], 31, 200, 3
    cfg = dict(world_width=8.0, world_height=8.0)
    off, on = tdm_twins(teams, E, seed, **cfg)
    fin = FinalBufs(on)
    act = combat_actions(off.obs, off.mask)
    acts = torch.empty((K + 1, E, 8, 4), dtype=torch.uint8, device=DEV)
    buf = on.trajectory_buffers(K)
    cap = Capture(E)
    by_combat, lengths = 0, set()
    for i in range(launches):
        n0 = len(cap.at)
        ref, arows = tdm_loop_bots_cap(off, act, K, cap, k0=i * K)
        acts[0] = act
        traj = on.rollout_bots_traj(acts, K, buf)
        assert_traj(ref, traj, f"launch {i}")
        assert torch.equal(acts, arows), f"launch {i}: action rows"
        act = arows[K].clone()
        fin.check(cap, f"launch {i}")
        # from the loop's rows: who ended how, and after how many steps
        winner = ref["winner"].cpu().numpy()
        by_combat += sum(int(winner[k - i * K, e] >= 0) for k, e in cap.at[n0:])
        lengths |= set(int(v) for v in cap.length[cap.ended])
    assert by_combat > 0, "some episode ended by combat"
    assert len({k for k, _ in cap.at}) > 1 and len(lengths) > 1, "ends on different steps, episodes of different lengths"
    assert int(cap.ends.sum()) == len(cap.at) > E
    assert_tdm_state(off, on)
    assert on.status() == 0


# ---- 6. the per-step path: workgroup rollouts, above 1024 agents ----------------------------------------
@pytest.mark.parametrize("bots", [False, True])
def test_flock_workgroup_path(bots):
    E, N, K = 4, 100, 20
    off, on = flock_twins(E, N, 23, time_limit=0.25, start_spread=12)
    fin = FinalBufs(on.world)
    cap = Capture(E)
    if bots:
        act0 = bot_flock(off.obs)
        ref, arows = flock_loop_bots_cap(off, act0, K, cap)
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        acts[0] = act0
        traj = on.rollout_bots(acts, K, trajectory=True)
        assert torch.equal(acts, arows)
    else:
        acts = flock_actions(K, E, N, 51)
        ref = flock_loop_cap(off, acts, cap)
        traj = on.rollout(acts, trajectory=True)
    assert_traj(ref, traj, "workgroup path")
    assert bool(traj["done"][15].all()) and (cap.ends == 1).all() and (cap.length == 16).all()
    fin.check(cap, "workgroup path")
    assert_flock_end(off, on, "workgroup path")


@pytest.mark.parametrize("bots", [False, True])
def test_tdm_workgroup_path(bots):
    E, teams, K, N = 4, [40, 40], 20, 80
    off, on = tdm_twins(teams, E, 11, time_limit=0.25)
    fin = FinalBufs(on)
    cap = Capture(E)
    if bots:
        act0 = combat_actions(off.obs, off.mask)
        ref, arows = tdm_loop_bots_cap(off, act0, K, cap)
        acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
        acts[0] = act0
        traj = on.rollout_bots_traj(acts, K)
        assert torch.equal(acts, arows)
    else:
        acts = tdm_random_actions(K, E, N, 8)
        ref = tdm_loop_cap(off, acts, cap)
        traj = on.rollout_traj(acts)
    assert_traj(ref, traj, "TDM workgroup path")
    assert bool(traj["done"][15].all()) and (cap.ends == 1).all() and (cap.length == 16).all()
    fin.check(cap, "TDM workgroup path")
    assert_tdm_state(off, on)


def test_flock_above_1024_agents():
    E, N, K = 2, 1025, 4
    # done when time_passed = n / 60 > time_limit: 2.5 / 60 ends an episode at its 3rd step
    off, on = flock_twins(E, N, 3, time_limit=2.5 / 60.0, start_spread=30)
    fin = FinalBufs(on.world)
    acts = flock_actions(K, E, N, 61)
    cap = Capture(E)
    ref = flock_loop_cap(off, acts, cap)
    traj = on.rollout(acts, trajectory=True)
    assert_traj(ref, traj, "N = 1025")
    assert traj["done"].cpu().numpy().tolist() == [[0] * E, [0] * E, [1] * E, [0] * E]
    assert (cap.ends == 1).all() and (cap.length == 3).all()
    fin.check(cap, "N = 1025")
    assert_flock_end(off, on, "N = 1025")


# ---- 7. partial registration and refusals --------------------------------------------------------------
def raw_flock_traj(w, acts, go):
    _abi.check(w.L.macm_world_rollout_traj(w.h, ctypes.c_void_p(acts.data_ptr()), int(acts.shape[0]), go.ref(),
                                           w._stream()), "macm_world_rollout_traj")


def test_only_length_and_ends_registered():
    """obs and nbr_id are NULL in the registration: their buffers keep FILL, and the call's own obs
    may be NULL."""
    E, N, K = 8, 64, 20
    off, on = flock_twins(E, N, 29, time_limit=0.25)
    fin = FinalBufs(on.world, fields=("length", "ends"))
    acts = flock_actions(K, E, N, 61)
    cap = Capture(E)
    ref = flock_loop_cap(off, acts, cap)
    go = GuardedOutputs(on.world, ("reward", "collided", "done"), n_steps=K)
    raw_flock_traj(on.world, acts, go)
    go.assert_equal(ref, "obs and nbr_id NULL")
    fin.check(cap, "length and ends only")
    assert (cap.ends == 1).all() and (cap.length == 16).all()
    assert_flock_end(off, on, "length and ends only", outputs=False)
    # TDM: out may be NULL altogether in the overwrite form
    toff, ton = tdm_twins([4, 4], E, 3, time_limit=0.25)
    tfin = FinalBufs(ton, fields=("length", "ends"))
    ta = tdm_random_actions(K, E, 8, 4)
    tcap = Capture(E)
    tdm_loop_cap(toff, ta, tcap)
    _abi.check(ton.L.macm_tdm_rollout(ton.h, ctypes.c_void_p(ta.data_ptr()), K, None, ton._stream()), "macm_tdm_rollout")
    tfin.check(tcap, "TDM, out NULL")
    assert_tdm_state(toff, ton)


def assert_state_unchanged(before, after):
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)


def test_registered_field_needs_the_calls_own_output():
    E, N, K = 4, 16, 3
    on = FlockVec(E, n_agents=[N], seed=1, device=DEV, autoreset=True)
    w = on.world
    acts = flock_actions(K, E, N, 1)
    ap, st = ctypes.c_void_p(acts.data_ptr()), w._stream()
    for fields, missing in ((("obs",), "obs"), (("nbr_id",), "nbr_id")):
        fin = FinalBufs(w, fields=fields)
        have = tuple(f for f in FKEYS if f != missing)
        one, many = GuardedOutputs(w, have), GuardedOutputs(w, have, n_steps=K)
        before = on.get_state()
        for name, call in (("macm_world_step", lambda: w.L.macm_world_step(w.h, ap, one.ref(), st)),
                           ("macm_world_rollout", lambda: w.L.macm_world_rollout(w.h, ap, K, one.ref(), st)),
                           ("macm_world_rollout_traj", lambda: w.L.macm_world_rollout_traj(w.h, ap, K, many.ref(), st))):
            with pytest.raises(MacmError, match=f"final outputs: {missing}") as ei:
                _abi.check(call(), name)
            assert ei.value.code == _abi.E_INVALID
        assert_state_unchanged(before, on.get_state())
        assert fin.all_fill()
        one.check_bands(missing)
        # with autoreset off the same calls are valid: nothing would be copied
        w.set_autoreset(False)
        _abi.check(w.L.macm_world_step(w.h, ap, one.ref(), st), "macm_world_step")
        w.set_autoreset(True)
    t = TdmWorld(tdm_config([4, 4]), E, device=DEV, autoreset=True)
    t.reset(1)
    ta = tdm_random_actions(K, E, 8, 1)
    tp, st = ctypes.c_void_p(ta.data_ptr()), t._stream()
    for fields, missing in ((("obs",), "obs"), (("mask",), "mask")):
        fin = FinalBufs(t, fields=fields)
        have = tuple(f for f in TKEYS if f != missing)
        one, many = GuardedOutputs(t, have), GuardedOutputs(t, have, n_steps=K)
        before = t.get_state()
        for name, call in (("macm_tdm_step", lambda: t.L.macm_tdm_step(t.h, tp, one.ref(), st)),
                           ("macm_tdm_rollout", lambda: t.L.macm_tdm_rollout(t.h, tp, K, one.ref(), st)),
                           ("macm_tdm_rollout", lambda: t.L.macm_tdm_rollout(t.h, tp, K, None, st)),
                           ("macm_tdm_rollout_traj", lambda: t.L.macm_tdm_rollout_traj(t.h, tp, K, many.ref(), st))):
            with pytest.raises(MacmError, match=f"final outputs: {missing}") as ei:
                _abi.check(call(), name)
            assert ei.value.code == _abi.E_INVALID
        assert_state_unchanged(before, t.get_state())
        assert fin.all_fill()


def test_misaligned_final_obs_is_refused():
    E, N = 4, 16
    on = FlockVec(E, n_agents=[N], seed=1, device=DEV, autoreset=True, time_limit=0.25)
    good = FinalBufs(on.world)
    bad = FinalBufs(on.world, register=False, zero_ends=False)
    bad.struct.obs = bad["obs"].data_ptr() + 4
    with pytest.raises(MacmError, match="16-byte") as ei:
        on.world._register_final(bad.struct)
    assert ei.value.code == _abi.E_INVALID
    t = TdmWorld(tdm_config([4, 4], time_limit=0.25), E, device=DEV, autoreset=True)
    tbad = FinalBufs(t, register=False, zero_ends=False)
    tbad.struct.obs = tbad["obs"].data_ptr() + 4
    with pytest.raises(MacmError, match="16-byte"):
        t._register_final(tbad.struct)
    # the refusal changed nothing: the earlier registration still receives the rows
    on.rollout(flock_actions(16, E, N, 2))
    torch.cuda.synchronize()
    assert bad.all_fill() and (good["ends"] == 1).all() and (good["length"] == 16).all()


@pytest.mark.parametrize("how", ["autoreset_off", "cleared"])
def test_nothing_is_written(how):
    """Autoreset off with buffers registered, and buffers cleared on an autoreset world: a rollout
    through an episode end leaves every final byte as it was."""
    E, N, K = 8, 64, 20
    vec = FlockVec(E, n_agents=[N], seed=37, device=DEV, time_limit=0.25, autoreset=how == "cleared")
    t = TdmWorld(tdm_config([16, 16], time_limit=0.25), 4, device=DEV, autoreset=how == "cleared")
    t.reset(5)
    fin, tfin = FinalBufs(vec.world, zero_ends=False), FinalBufs(t, zero_ends=False)
    if how == "cleared":
        vec.world.set_final_outputs(False)
        t.set_final_outputs(False)
    traj = vec.rollout(flock_actions(K, E, N, 71), trajectory=True)
    ttraj = t.rollout_traj(tdm_random_actions(K, 4, 32, 2))
    for k in range(3):
        vec.step(flock_actions(1, E, N, 72 + k)[0])
    assert bool(traj["done"][15].all()) and bool(ttraj["done"][15].all())
    assert fin.all_fill() and tfin.all_fill()


# ---- 8. the Python handles -----------------------------------------------------------------------------
def test_python_handles_own_the_tensors():
    E, N, K = 4, 20, 16
    off = FlockVec(E, n_agents=[N], seed=2, device=DEV, time_limit=0.25)
    on = FlockVec(E, n_agents=[N], seed=2, device=DEV, time_limit=0.25, autoreset=True, final_obs=True)
    assert on.final_obs.shape == on.obs.shape and on.final_obs.dtype == on.obs.dtype
    assert int(on.final_ends.sum()) == 0 and int(on.final_length.sum()) == 0
    acts = flock_actions(K, E, N, 3)
    cap = Capture(E)
    flock_loop_cap(off, acts, cap)
    obs, nbr, rew, done = on.rollout(acts)
    assert bool(done.all())
    assert torch.equal(bits(on.final_obs), bits(cap.rows["obs"])) and torch.equal(on.final_nbr_id, cap.rows["nbr_id"])
    assert torch.equal(bits(on.final_obs[done.bool()]), bits(cap.rows["obs"]))  # info["terminal_observation"]
    assert (on.final_ends == 1).all() and (on.final_length == 16).all()
    on.world.set_final_outputs(False)
    assert on.final_obs is None and on.final_ends is None
    toff, ton = TdmWorld(tdm_config([4, 4], time_limit=0.25), E, device=DEV), \
        TdmWorld(tdm_config([4, 4], time_limit=0.25), E, device=DEV, autoreset=True, final_obs=True)
    toff.reset(4)
    ton.reset(4)
    ta = tdm_random_actions(K, E, 8, 6)
    tcap = Capture(E)
    tdm_loop_cap(toff, ta, tcap)
    for k in range(K):
        ton.step(ta[k])
    # values, not bits: the loop's step() takes the split observation here (fused_observation above)
    assert torch.equal(ton.final_obs, tcap.rows["obs"]) and torch.equal(ton.final_mask, tcap.rows["mask"])
    assert (ton.final_ends == 1).all() and (ton.final_length == 16).all()
