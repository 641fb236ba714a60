"""TDM combat events (macm_tdm_set_events, TdmWorld.set_events) on the device.

hit_id[e, i] = the body agent i's attack damaged in the step, or -1, is compared with the events
derived from the CPU oracle (tdm_events_ref: the oracle's pre-step states and the same actions, the
replay checked against the oracle by test_tdm_events_ref.py), bit for bit, in every call form; and a
twin world without events, given the same calls, must give every existing output, the final
get_state, the counters and spilled bit for bit, since a world with events launches kernels of its own."""
import ctypes
import random

import numpy as np
import pytest
import torch
from guard_bands import Guarded, GuardedOutputs
from test_gpu_tdm_split import same_tensor  # obs on bit patterns, the rest on values
from tdm_events_ref import FIXTURES, fixture_actions, fixture_config, replay, run_fixture

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.tdm_world import TdmWorld  # noqa: E402

OUT = TdmWorld._TRAJ_KEYS
DEV = "cuda:0"


def worlds(name, n=2, events=(True, False), **kw):
    """Worlds of a fixture after reset(seed): by default one with events and its twin without."""
    _, E, _, seed, _, _ = FIXTURES[name]
    ws = []
    for ev in events[:n]:
        w = TdmWorld(fixture_config(name), E, device=DEV, events=ev, **kw)
        w.reset(seed)
        ws.append(w)
    return ws


def dev_actions(name):
    return torch.from_numpy(fixture_actions(name)).to(DEV)


def hits(t):
    return t.cpu().numpy()


def assert_twins(a, b, ctx, outputs=True, counters=True):
    """Everything a world had before events existed: outputs, state, counters, spilled, status.
    (counters=False: worlds that were not given the same calls; the counters run on across reset().)"""
    torch.cuda.synchronize()
    if outputs:
        for k in OUT:
            assert same_tensor(getattr(a, k), getattr(b, k), k), f"{ctx}: output {k} differs from the twin's"
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{ctx}: state[{k}]")
    if counters:
        np.testing.assert_array_equal(a.counters(), b.counters(), err_msg=f"{ctx}: counters")
        assert a.spilled() == b.spilled(), f"{ctx}: spilled"
    assert a.status() == 0 and b.status() == 0, ctx


def assert_traj_twins(ta, tb, ctx):
    for k in OUT:
        assert same_tensor(ta[k], tb[k], k), f"{ctx}: trajectory {k} differs from the twin's"


def step_loop(w, acts, reset):
    """step K times (reset: reset_envs(done) after each step, the loop autoreset replaces); the
    hit_id rows (None without events) and the terminal health / alive / done / winner rows."""
    rows, term = [], {k: [] for k in ("health", "alive", "done", "winner")}
    for a in acts:
        w.step(a)
        if w.hit_id is not None:
            rows.append(w.hit_id.clone())
        for k in term:
            term[k].append(getattr(w, k).clone())
        if reset:
            w.reset_envs(w.done.clone())
            if w.hit_id is not None:  # a reset writes no events: the terminal step's stay
                assert torch.equal(w.hit_id, rows[-1])
    return (torch.stack(rows) if rows else None), {k: torch.stack(v) for k, v in term.items()}


# ---- 1. parity with the derived events, and with a twin without events -------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_step_matches_the_reference(name):
    ref, reset = run_fixture(name), FIXTURES[name][5]
    w, twin = worlds(name)
    assert w.hit_id.dtype == torch.int32 and tuple(w.hit_id.shape) == (w.E, w.N) and bool((w.hit_id == -1).all())
    acts = dev_actions(name)
    got, term = step_loop(w, acts, reset)
    _, tterm = step_loop(twin, acts, reset)
    for k in range(acts.shape[0]):
        np.testing.assert_array_equal(hits(got[k]), ref["hit_id"][k], err_msg=f"{name}: hit_id of step {k}")
    for k in term:
        assert torch.equal(term[k], tterm[k]), f"{name}: {k} rows differ from the twin's"
        np.testing.assert_array_equal(term[k].cpu().numpy(), ref[k], err_msg=f"{name}: {k} against the oracle")
    assert_twins(w, twin, f"{name} step")


NO_RESET = [n for n in FIXTURES if not FIXTURES[n][5]]


@pytest.mark.parametrize("name", NO_RESET)
def test_rollouts_match_the_reference(name):
    ref = run_fixture(name)
    acts = dev_actions(name)
    K = acts.shape[0]
    w, twin = worlds(name)
    w.rollout(acts)
    twin.rollout(acts)
    np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][K - 1], err_msg=f"{name}: rollout leaves the last step's")
    assert_twins(w, twin, f"{name} rollout")
    # the trajectory form from a fresh episode: every row, and the world's own tensor keeps the last
    w.reset(FIXTURES[name][3])
    twin.reset(FIXTURES[name][3])
    traj = w.rollout_traj(acts)
    ttraj = twin.rollout_traj(acts)
    assert "hit_id" in traj and "hit_id" not in ttraj and tuple(traj["hit_id"].shape) == (K, w.E, w.N)
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"], err_msg=f"{name}: rollout_traj rows")
    assert torch.equal(w.hit_id, traj["hit_id"][K - 1])
    np.testing.assert_array_equal(traj["health"].cpu().numpy(), ref["health"])
    assert_traj_twins(traj, ttraj, f"{name} rollout_traj")
    assert_twins(w, twin, f"{name} rollout_traj")
    # the world's own registration is back: a step writes its [E, N] tensor, not the trajectory's rows
    keep = traj["hit_id"].clone()
    w.step(acts[0])
    twin.step(acts[0])
    assert torch.equal(traj["hit_id"], keep)
    assert_twins(w, twin, f"{name} step after rollout_traj")


# ---- 2. the closed loop -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W1", "G1"])
def test_closed_loop(name):
    _, E, K, seed, _, _ = FIXTURES[name]
    w, twin = worlds(name)
    N = w.N
    a0 = dev_actions(name)[0]
    acts = torch.zeros((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
    tacts = acts.clone()
    acts[0], tacts[0] = a0, a0
    traj = w.rollout_bots_traj(acts, K)
    ttraj = twin.rollout_bots_traj(tacts, K)
    assert torch.equal(acts, tacts)
    # the reference: the oracle through the actions the call left in its [K + 1, E, N, 4] buffer
    ref = replay(fixture_config(name, obs_f64=True), E, seed, acts[:K].cpu().numpy(), False)
    assert int((ref["hit_id"] >= 0).sum()) >= 20, "the bots must land hits for this to test anything"
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"], err_msg=f"{name}: rollout_bots_traj rows")
    np.testing.assert_array_equal(traj["health"].cpu().numpy(), ref["health"])
    assert_traj_twins(traj, ttraj, f"{name} rollout_bots_traj")
    assert_twins(w, twin, f"{name} rollout_bots_traj")
    # the overwrite form: row 0 holds the last step's
    w.reset(seed)
    twin.reset(seed)
    a, ta = a0.clone(), a0.clone()
    w.rollout_bots(a, K)
    twin.rollout_bots(ta, K)
    assert torch.equal(a, ta) and torch.equal(a, acts[K])
    np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][K - 1], err_msg=f"{name}: rollout_bots")
    assert_twins(w, twin, f"{name} rollout_bots")


# ---- 3. launch forms ----------------------------------------------------------------------------------
FORMS = {"default": {}, "fused": {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "0"},
         "split": {"MACM_TDM_SPLIT_OBS": "1", "MACM_TDM_TAIL_OBS": "0"}}


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_forms_give_the_same_events(form, monkeypatch):
    for k in ("MACM_TDM_SPLIT_OBS", "MACM_TDM_TAIL_OBS", "MACM_TDM_TAIL_WORKERS", "MACM_TDM_TAIL_STEPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    ref = run_fixture("W1")
    acts = dev_actions("W1")
    w, twin = worlds("W1")
    want = {"default": _abi.LAUNCH_SPLIT_OBS | _abi.LAUNCH_TAIL_OBS, "fused": 0, "split": _abi.LAUNCH_SPLIT_OBS}[form]
    assert w.launch_flags() == want and twin.launch_flags() == want, (form, w.launch_flags())
    # the 40-step trajectory: the tail observation (default), one fused launch, or split chunks of 8
    traj, ttraj = w.rollout_traj(acts), twin.rollout_traj(acts)
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"], err_msg=f"{form}: rollout_traj rows")
    assert_traj_twins(traj, ttraj, f"{form} rollout_traj")
    assert_twins(w, twin, f"{form} rollout_traj")
    # step and the overwrite rollout: the split observation (default, split) or fused
    w.reset(3)
    twin.reset(3)
    for k in range(6):
        w.step(acts[k])
        twin.step(acts[k])
        np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][k], err_msg=f"{form}: step {k}")
    w.rollout(acts[6:])
    twin.rollout(acts[6:])
    np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][-1], err_msg=f"{form}: rollout after steps")
    assert_twins(w, twin, f"{form} step + rollout")


def test_forced_spill_step_gives_the_same_events():
    """The wave kernel hands every env to the spill step after the casts (MACM_DEBUG_FORCE_SPILL):
    the events are stored with the combat state committed before the hand-over."""
    ref = run_fixture("W1")
    acts = dev_actions("W1")
    w, twin = worlds("W1")
    w.set_debug(_abi.DEBUG_FORCE_SPILL)
    twin.set_debug(_abi.DEBUG_FORCE_SPILL)
    traj, ttraj = w.rollout_traj(acts[:12]), twin.rollout_traj(acts[:12])
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"][:12])
    for k in range(12, 16):
        w.step(acts[k])
        twin.step(acts[k])
        np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][k], err_msg=f"step {k}")
    assert w.spilled() == 16 * w.E
    assert_traj_twins(traj, ttraj, "forced spill")
    assert_twins(w, twin, "forced spill")
    # W5: with the in-launch reset between the steps
    ref = run_fixture("W5")
    acts = dev_actions("W5")
    w, twin = worlds("W5", autoreset=True)
    w.set_debug(_abi.DEBUG_FORCE_SPILL)
    twin.set_debug(_abi.DEBUG_FORCE_SPILL)
    traj, ttraj = w.rollout_traj(acts), twin.rollout_traj(acts)
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"])
    assert w.spilled() == acts.shape[0] * w.E
    assert_traj_twins(traj, ttraj, "forced spill, autoreset")
    assert_twins(w, twin, "forced spill, autoreset")


# ---- 4. autoreset ---------------------------------------------------------------------------------------
AR = {"W5": {}, "W6": {}, "G1": dict(time_limit=0.1)}


def ar_worlds(name):
    """(events + autoreset, autoreset without events, events without autoreset: the loop's)"""
    _, E, _, seed, _, _ = FIXTURES[name]
    ws = []
    for ev, ar in ((True, True), (False, True), (True, False)):
        w = TdmWorld(fixture_config(name, **AR[name]), E, device=DEV, events=ev, autoreset=ar)
        w.reset(seed)
        ws.append(w)
    return ws


@pytest.mark.parametrize("name", list(AR))
def test_autoreset_given_actions(name):
    _, E, K, seed, _, _ = FIXTURES[name]
    acts = dev_actions(name)
    ref = (run_fixture(name) if not AR[name] else
           replay(fixture_config(name, obs_f64=True, **AR[name]), E, seed, fixture_actions(name), True))
    ends = int(ref["done"].sum())
    assert ends >= 1 and int((ref["hit_id"] >= 0).sum()) >= 100
    w, twin, loop = ar_worlds(name)
    # the loop step -> reset_envs(done) that autoreset replaces: its rows are the reference's
    lrows, lterm = step_loop(loop, acts, True)
    np.testing.assert_array_equal(hits(lrows), ref["hit_id"], err_msg=f"{name}: the loop")
    # step with autoreset on: the terminal row keeps the step's events
    got, term = step_loop(w, acts, False)
    _, tterm = step_loop(twin, acts, False)
    assert torch.equal(got, lrows), f"{name}: step with autoreset against the loop"
    for k in term:
        assert torch.equal(term[k], lterm[k]) and torch.equal(term[k], tterm[k]), f"{name}: {k}"
    assert_twins(w, twin, f"{name} autoreset step", outputs=False)
    assert_twins(w, loop, f"{name} autoreset step against the loop", outputs=False)
    # the rollouts, each from a fresh episode
    for form in ("rollout", "rollout_traj"):
        w.reset(seed)
        twin.reset(seed)
        if form == "rollout":
            w.rollout(acts)
            twin.rollout(acts)
            np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][K - 1], err_msg=f"{name}: rollout")
        else:
            traj, ttraj = w.rollout_traj(acts), twin.rollout_traj(acts)
            np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"], err_msg=f"{name}: rollout_traj")
            np.testing.assert_array_equal(traj["done"].cpu().numpy(), ref["done"])
            assert_traj_twins(traj, ttraj, f"{name} autoreset rollout_traj")
        assert_twins(w, twin, f"{name} autoreset {form}")
        assert_twins(w, loop, f"{name} autoreset {form} against the loop", outputs=False, counters=False)
    if name == "W6":  # the first attacks after a reset see a fresh listener: nothing damaged before a ray hits
        after = np.argwhere(ref["done"][:-1] != 0)
        assert len(after) >= 32
        for k, e in after:
            row, rays = ref["hit_id"][k + 1, e], ref["ray_hit"][k + 1, e]
            first = np.flatnonzero(rays >= 0)
            upto = first[0] if len(first) else len(row)
            assert (traj["hit_id"][k + 1, e, :upto].cpu().numpy() == -1).all() and (row[:upto] == -1).all()


@pytest.mark.parametrize("name", ["W5", "W6", "G1"])
def test_autoreset_closed_loop(name):
    _, E, K, seed, _, _ = FIXTURES[name]
    w, twin, _ = ar_worlds(name)
    N = w.N
    a0 = dev_actions(name)[0]
    acts = torch.zeros((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
    tacts = acts.clone()
    acts[0], tacts[0] = a0, a0
    traj, ttraj = w.rollout_bots_traj(acts, K), twin.rollout_bots_traj(tacts, K)
    assert torch.equal(acts, tacts)
    ref = replay(fixture_config(name, obs_f64=True, **AR[name]), E, seed, acts[:K].cpu().numpy(), True)
    np.testing.assert_array_equal(hits(traj["hit_id"]), ref["hit_id"], err_msg=f"{name}: rollout_bots_traj")
    np.testing.assert_array_equal(traj["done"].cpu().numpy(), ref["done"])
    assert_traj_twins(traj, ttraj, f"{name} autoreset rollout_bots_traj")
    assert_twins(w, twin, f"{name} autoreset rollout_bots_traj")
    w.reset(seed)
    twin.reset(seed)
    a, ta = a0.clone(), a0.clone()
    w.rollout_bots(a, K)
    twin.rollout_bots(ta, K)
    assert torch.equal(a, ta) and torch.equal(a, acts[K])
    np.testing.assert_array_equal(hits(w.hit_id), ref["hit_id"][K - 1], err_msg=f"{name}: rollout_bots")
    assert_twins(w, twin, f"{name} autoreset rollout_bots")


# ---- 5. guards ------------------------------------------------------------------------------------------
def register(w, g, rows):
    ev = _abi.MacmTdmEvents(ctypes.c_void_p(g.t.data_ptr()), rows)
    _abi.check(w.L.macm_tdm_set_events(w.h, ctypes.byref(ev)), "macm_tdm_set_events")


def all_rows(g, value):
    return np.full(g.t.shape[0], value, bool)


@pytest.mark.parametrize("name", ["W1", "G1"])
def test_nothing_is_written_outside_the_rows(name):
    """Through the C-ABI with the events in a guarded buffer of 3 rows."""
    ref = run_fixture(name)
    acts = dev_actions(name)
    (w,) = worlds(name, n=1, events=(False,))
    g = Guarded((3, w.E, w.N), torch.int32)
    register(w, g, 3)
    out = GuardedOutputs(w, ("health", "done"))
    # a step writes row 0 and nothing else
    _abi.check(w.L.macm_tdm_step(w.h, ctypes.c_void_p(acts[0].data_ptr()), out.ref(), w._stream()), "step")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hits(g.t[0]), ref["hit_id"][0])
    assert g.bands_intact() and g.rows_untouched([False, True, True])
    # a trajectory of more steps than rows is refused and steps nothing
    before = w.get_state()
    tout = GuardedOutputs(w, ("health", "done"), n_steps=4)
    rc = w.L.macm_tdm_rollout_traj(w.h, ctypes.c_void_p(acts[1:5].data_ptr()), 4, tout.ref(), w._stream())
    assert rc == _abi.E_INVALID and b"rows" in w.L.macm_last_error()
    after = w.get_state()
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=f"refused call changed state[{k}]")
    assert g.rows_untouched([False, True, True])
    # three steps fill the three rows; the overwrite rollout then writes row 0 alone
    _abi.check(w.L.macm_tdm_rollout_traj(w.h, ctypes.c_void_p(acts[1:4].data_ptr()), 3, tout.ref(), w._stream()), "traj")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hits(g.t), ref["hit_id"][1:4])
    _abi.check(w.L.macm_tdm_rollout(w.h, ctypes.c_void_p(acts[4:7].data_ptr()), 3, out.ref(), w._stream()), "rollout")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hits(g.t[0]), ref["hit_id"][6])
    np.testing.assert_array_equal(hits(g.t[1:]), ref["hit_id"][2:4])
    assert g.bands_intact()
    out.check_bands(name)
    tout.check_bands(name)
    # calls that are no step write no events; nor does anything once the registration is cleared
    g2 = Guarded((3, w.E, w.N), torch.int32)
    register(w, g2, 3)
    w.observe()
    w.reset_envs(torch.ones(w.E, dtype=torch.uint8, device=DEV))
    st = w.get_state()
    w.place(st["pos"], st["angle"])
    w.reset(FIXTURES[name][3])
    torch.cuda.synchronize()
    assert g2.rows_untouched(all_rows(g2, True)) and g2.bands_intact()
    _abi.check(w.L.macm_tdm_set_events(w.h, None), "macm_tdm_set_events")
    w.step(acts[0])
    w.rollout_traj(acts[1:4])
    torch.cuda.synchronize()
    assert g2.rows_untouched(all_rows(g2, True)) and g2.bands_intact()
    np.testing.assert_array_equal(w.health.cpu().numpy(), ref["health"][3])


@pytest.mark.parametrize("name", ["W1", "G1"])
def test_unstepped_envs_keep_their_rows(name):
    """MACM_DEBUG_SPILL_FAIL: no env gets a working-set slot, every env is left unstepped
    (MACM_ST_SPILL_WAIT) and its row of events untouched, as its health output is."""
    acts = dev_actions(name)
    (w,) = worlds(name, n=1, events=(False,))
    w.step(acts[0])
    g = Guarded((2, w.E, w.N), torch.int32)
    register(w, g, 2)
    w.set_debug(_abi.DEBUG_FORCE_SPILL | _abi.DEBUG_SPILL_FAIL)
    w.step(acts[1])
    torch.cuda.synchronize()
    assert w.status() & _abi.ST_SPILL_WAIT
    assert g.rows_untouched(all_rows(g, True)) and g.bands_intact()


def test_host_outputs_and_the_dict_api():
    """hit_id in pinned host memory (host_outputs), and gym_macm.envs.TDM.hits from it."""
    ref = run_fixture("W3")
    _, E, K, seed, _, _ = FIXTURES["W3"]
    w = TdmWorld(fixture_config("W3"), E, device=DEV, host_outputs=True, events=True)
    w.reset(seed)
    assert w.hit_id.is_pinned() and w.hit_id.device.type == "cpu"
    acts = dev_actions("W3")
    for k in range(K):
        w.step(acts[k])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(w.hit_id.numpy(), ref["hit_id"][k], err_msg=f"pinned hit_id, step {k}")

    from gym_macm.envs import TDM
    seed, K, teams = 21, 40, [8, 8]
    random.seed(seed)
    env = TDM(n_agents=teams, cooldown_atk=0.05)
    assert env.hits == {} and env.get_rewards() is None
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.integers(0, 3, (K, 16, 3)), rng.integers(0, 2, (K, 16, 1))], axis=-1).astype(np.uint8)
    dref = replay(env.world.cfg, 1, seed, a[:, None], False)
    assert int((dref["hit_id"] >= 0).sum()) >= 20
    ids = [agent.id for agent in env.agents]
    for k in range(K):
        env.step({agent.id: a[k, i] for i, agent in enumerate(env.agents) if agent.alive})
        want = {ids[i]: ids[v] for i, v in enumerate(dref["hit_id"][k, 0]) if v >= 0}
        assert env.hits == want, (k, env.hits, want)
        assert env.get_rewards() is None
