"""Every writer of TDM's [N, N-1, 4] observation against tests/tdm_obs_ref.py, bit for bit.

Six code paths write the observation and each claims the same bits as the others (csrc/tdm_obs.hpp,
csrc/tdm_obs_snap.hip):

    rowblocks        tdm_obs_rowblocks, LDS stage     fused wave step, float32 obs, 9 <= N <= 32
    rowblocks/pieces the same with mask_pieces        tail observation (trajectory rollouts)
    pairs            tdm_obs_pairs                    fused wave step (float64 obs, N <= 8 or 33 <= N <= 64),
                                                      wave reset / observe(), spill step N <= 64, tail rows not staged
    snap             tdm_observe_snap                 split observation
    block            tdm_obs_block (pair round robin) reset / observe() at N > 64
    linear           tdm_obs_block_linear             workgroup step, spill step "wide"

The comparisons elsewhere in the suite (parity.f32_obs_mismatch, tdm_obs_close, torch.equal) allow an
ulp or are blind to the sign of a zero. Here every observation is compared with the host restatement
on uint32 / uint64 views and the mask as bytes; the restatement is computed from the oracle's state
after each step, whose positions, angles and alive flags the device reproduces exactly (asserted
first). tests/test_tdm_obs_ref.py holds the restatement to the oracle.

Worlds: (a) crowded random rollouts with deaths, so masked slots occur; (b) constructed states
(constructed.inject_tdm) that put equal angles, +-float32(pi), shared x, shared y, |rx| == |ry| and
dead agents into the same 8-block, different 8-blocks and the diagonal tiles, with one env whose
deaths cross the blocks, one with a whole team dead and one with a single survivor (every mask byte
and every observation bit zero); (c) short random rollouts from reset at every N. Where the library
reports the form it took (launch_flags(), spilled()) the test asserts it.

Before the fix of this file's commit two differences showed: the row-block stage wrote p = -0.0f into
masked slots (float32, 9 <= N <= 32, a dead agent), and the pair form's reverse direction gave
p = -0.0 for equal angles where the slot-by-slot writers give +0.0."""
import numpy as np
import pytest
import torch

from constructed import inject_tdm
from oracle import OracleTDM
from tdm_obs_ref import as_bits, assert_same_mask_bytes, assert_same_obs_bits, tdm_obs  # noqa: F401  (fixture)
from test_math_forms import forms  # noqa: F401  (fixture: macm_math.h built for the host)

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402

PI32 = np.float32(np.pi)
TEAMS = {2: [1, 1], 8: [4, 4], 9: [5, 4], 10: [5, 5], 16: [8, 8], 32: [16, 16], 33: [17, 16], 64: [32, 32],
         65: [33, 32], 130: [44, 43, 43]}
FUSED = {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "0"}
SPLIT = {"MACM_TDM_SPLIT_OBS": "1", "MACM_TDM_TAIL_OBS": "0"}
TAIL = {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "1"}
FORM_VARS = ("MACM_TDM_SPLIT_OBS", "MACM_TDM_TAIL_OBS", "MACM_TDM_TAIL_WORKERS", "MACM_TDM_TAIL_STEPS")


# ---- the worlds -----------------------------------------------------------------------------------------

def constructed_state(teams):
    """pos [4, N, 2], angle [4, N], alive [4, N] of the constructed world: bodies on a lattice of 1.5 m (no
    contacts, so idle bodies stay where they are), six to a row, so that agents of one 8-block and of
    neighbouring blocks share y, agents i and i + 6 share x and the lattice's diagonals have
    |rx| == |ry|; env 1 is the transposed lattice. Angles from a palette in which agents (0, 1, 7, 8)
    are equal (allies and enemies, same block and across blocks) and +-float32(pi) meet in one
    block (3, 5) and across blocks (5, 10), (3, 12). Deaths: env 0 none; env 1 agents 1 and 2 (block 0:
    their partners in block 1), agent 9 (block 1: partners in block 0) and the last agent; env 2 the
    whole first team; env 3 everyone but one agent."""
    N, E = sum(teams), 4
    i = np.arange(N)
    lat = np.stack([1.5 * (i % 6), 1.5 * (i // 6)], -1).astype(np.float32)
    pos = np.stack([lat, lat[:, ::-1], 1.5 * np.stack([i % 5, i // 5], -1).astype(np.float32), lat])
    pal = np.array([0.7, PI32, -PI32, 0.7, -2.5, 0.0, 1.25], np.float32)
    ang = np.stack([pal[(3 * i + e) % 7] for e in range(E)]).astype(np.float32)
    alive = np.ones((E, N), np.uint8)
    if N == 2:  # env 0 equal angles, env 1 +-pi, env 2 the first team dead, env 3 the last agent dead
        ang = np.array([[0.7, 0.7], [PI32, -PI32], [-PI32, PI32], [0.7, 0.7]], np.float32)
        alive[2, 0] = 0
        alive[3, 1] = 0
    else:
        alive[1, [k for k in (1, 2, 9, N - 1) if k < N]] = 0
        alive[2, :teams[0]] = 0
        alive[3] = 0
        alive[3, N // 2] = 1
    return pos, ang, alive


WORLDS = {  # name: (teams, E, seed, config keywords, steps, p_attack)
    "crowded10": ([5, 5], 4, 11, dict(world_width=6.0, world_height=6.0), 40, 0.5),
    "crowded16": ([8, 8], 4, 11, dict(world_width=8.0, world_height=8.0), 40, 0.5),
}
for _n, _t in TEAMS.items():
    _kw = dict(world_width=20.0, world_height=20.0) if _n > 64 else {}
    WORLDS[f"reset{_n}"] = (_t, 3, 100 + _n, _kw, 8, 0.5)
    WORLDS[f"built{_n}"] = (_t, 4, 200 + _n, dict(world_width=30.0, world_height=30.0), 34 if _n <= 64 else 9, 0.5)
_REF = {}


def reference(tdm_obs, name):  # noqa: F811
    """The oracle's rollout of a world, once, shared by every case that runs the world: the state to inject
    (built worlds), the actions, and after t = 0 .. steps steps the state's pos / angle / alive / health /
    done / winner with the expected observation in both widths and the mask. Read-only."""
    if name in _REF:
        return _REF[name]
    teams, E, seed, kw, steps, p_attack = WORLDS[name]
    N = sum(teams)
    orc = OracleTDM(tdm_config(teams, obs_f64=True, **kw), E, seed)
    rng = np.random.default_rng(seed)
    acts = rng.integers(0, 3, size=(steps, E, N, 4)).astype(np.uint8)
    acts[..., 3] = rng.random((steps, E, N)) < p_attack
    st0 = None
    if name.startswith("built"):
        pos, ang, alive = constructed_state(teams)
        inject_tdm(None, orc, pos, ang, alive=alive, health=alive.astype(np.float64))
        st0 = orc.get_state()
        assert (as_bits(st0["pos"]) == as_bits(pos)).all() and (as_bits(st0["angle"]) == as_bits(ang)).all()
        acts[0] = (1, 1, 1, 0)  # one idle step first

    def row(o_mask):
        st = orc.get_state()
        o32, o64, m = tdm_obs(st["pos"], st["angle"], st["alive"], teams)
        np.testing.assert_array_equal(m, o_mask, err_msg=f"{name}: the restatement's mask against the oracle's")
        return dict(o32=o32, o64=o64, mask=m, pos=st["pos"], angle=st["angle"], alive=st["alive"],
                    health=st["health"], done=st["done"], winner=st["winner"])

    rows = [row(orc.observe()[1])]
    for t in range(steps):
        rows.append(row(orc.step(acts[t])["mask"]))
    ref = dict(name=name, teams=teams, E=E, N=N, seed=seed, kw=kw, steps=steps, acts=acts, st0=st0, rows=rows)
    for r in rows:
        for v in r.values():
            v.setflags(write=False)
    acts.setflags(write=False)
    _REF[name] = ref
    return ref


# ---- running a world on the device ------------------------------------------------------------------------

def set_form(monkeypatch, env):
    for k in FORM_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def clear_form(monkeypatch):
    for k in FORM_VARS:
        monkeypatch.delenv(k, raising=False)


def make_world(ref, f64, debug=0):
    w = TdmWorld(tdm_config(ref["teams"], obs_f64=f64, **ref["kw"]), ref["E"], device="cuda:0")
    if debug:
        w.set_debug(debug)
    w.reset(ref["seed"], 0)
    return w


def same_obs(ref, t, obs, mask, f64, ctx, found=None):
    """obs and mask against the reference's row after t steps. found: a list that takes the message of a
    difference instead of raising it, so that one run reports every writer of a plan (run() raises them)."""
    row = ref["rows"][t]
    try:
        assert_same_mask_bytes(mask.cpu().numpy(), row["mask"], ctx)
        assert_same_obs_bits(obs.cpu().numpy(), row["o64" if f64 else "o32"], ctx, row["mask"], row["angle"])
    except AssertionError as e:
        if found is None:
            raise
        found.append(str(e))


def same_state(ref, t, w, ctx):
    """Positions, angles and alive of the device world are the oracle's after t steps, on bits."""
    row, s = ref["rows"][t], w.get_state()
    for k in ("pos", "angle", "alive", "health"):
        assert (as_bits(s[k]) == as_bits(row[k])).all(), f"{ctx}: state[{k}] differs from the oracle's"


def run(ref, w, plan, writer, step_writer=None):
    """Run `plan` on world w, a list of (kind, steps): "reset" (the observation reset() wrote), "observe",
    "steps" (per-step launches), "rollout" (one overwrite launch: the last step's outputs) and "traj" (one
    trajectory launch); every observation compared with the reference's row. The state is asserted as the
    plan goes; observation differences are gathered and raised together at the end, each naming its writer
    (reset() and observe() write with the pair form whatever the step's writer is; step_writer: the writer
    of step() and rollout() where the trajectory's is another, as for the tail observation). Returns the
    steps taken."""
    f64 = bool(w.cfg.obs_f64)
    step_writer = step_writer or writer
    own = "pairs" if ref["N"] <= 64 else "block"
    acts = torch.from_numpy(ref["acts"].copy()).cuda()
    t, found = 0, []
    if ref["st0"] is not None:
        w.set_state(ref["st0"])
    for kind, k in plan:
        if kind == "reset":
            assert t == 0 and ref["st0"] is None
            same_obs(ref, 0, w.obs, w.mask, f64, f"reset() ({own})", found)
        elif kind == "observe":
            w.observe()
            same_state(ref, t, w, f"before observe() after {t} steps")
            same_obs(ref, t, w.obs, w.mask, f64, f"observe() ({own}) after {t} steps", found)
        elif kind == "steps":
            for _ in range(k):
                w.step(acts[t])
                t += 1
                same_state(ref, t, w, f"{step_writer} step {t - 1}")
                same_obs(ref, t, w.obs, w.mask, f64, f"{step_writer} per-step launch, step {t - 1}", found)
        elif kind == "rollout":
            w.rollout(acts[t:t + k])
            t += k
            same_state(ref, t, w, f"{step_writer} overwrite rollout to step {t - 1}")
            same_obs(ref, t, w.obs, w.mask, f64, f"{step_writer} overwrite rollout of {k}, step {t - 1}", found)
        elif kind == "traj":
            tr = w.rollout_traj(acts[t:t + k])
            for s in range(k):
                row = ref["rows"][t + s + 1]
                assert (tr["alive"][s].cpu().numpy() == row["alive"]).all(), f"{writer} trajectory step {t + s}: alive"
                assert (as_bits(tr["health"][s].cpu().numpy()) == as_bits(row["health"])).all(), \
                    f"{writer} trajectory step {t + s}: health"
                same_obs(ref, t + s + 1, tr["obs"][s], tr["mask"][s], f64, f"{writer} trajectory of {k}, step {t + s}", found)
            t += k
            same_state(ref, t, w, f"{writer} trajectory to step {t - 1}")
            same_obs(ref, t, w.obs, w.mask, f64, f"{writer} trajectory of {k}: the world's own outputs", found)
        else:
            raise ValueError(kind)
    assert w.status() == 0
    assert not found, f"{ref['name']}: {len(found)} observations differ from the reference:\n" + "\n".join(found[:6])
    return t


def flags(w):
    return w.launch_flags() & (_abi.LAUNCH_SPLIT_OBS | _abi.LAUNCH_TAIL_OBS)


def plans_for(name, traj):
    """The per-launch plan and the overwrite-rollout plan of a world."""
    steps = WORLDS[name][4]
    if name.startswith("built"):  # observe(), one idle step, a short trajectory; the same steps in one overwrite launch
        return [("observe", 0), ("steps", 1), ("traj", traj)], [("rollout", 1 + traj)]
    if name.startswith("reset"):
        return [("reset", 0), ("observe", 0), ("steps", steps)], [("rollout", steps)]
    return [("steps", steps)], [("rollout", 8)] * (steps // 8)


def some_dead(ref, t):
    assert (ref["rows"][t]["alive"] == 0).any(), f"{ref['name']}: nobody dead after {t} steps, no masked slot compared"


# ---- the fused wave step ----------------------------------------------------------------------------------

FUSED_F32 = [f"{k}{n}" for n in (2, 8, 9, 10, 16, 32, 33, 64) for k in ("built", "reset")] + ["crowded10", "crowded16"]


def fused_writer(N, f64):
    return "fused wave step, " + ("float64: pairs" if f64 else "float32: " + ("rowblocks" if 9 <= N <= 32 else "pairs"))


@pytest.mark.parametrize("name", FUSED_F32)
def test_fused_wave_step_f32(monkeypatch, tdm_obs, name):  # noqa: F811
    """N = 2, 8: one block, nothing staged; 9, 10: a second block of 1 and 2 rows; 16, 32: whole blocks;
    33, 64: the pair tiles, partial and full last tile, both halves of the diagonal passes."""
    ref = reference(tdm_obs, name)
    set_form(monkeypatch, FUSED)
    per_launch, overwrite = plans_for(name, 5)
    for plan in (per_launch, overwrite):
        w = make_world(ref, False)
        assert flags(w) == 0
        t = run(ref, w, plan, fused_writer(ref["N"], False))
        assert w.spilled() == 0
    if not name.startswith("reset"):
        some_dead(ref, t)
    clear_form(monkeypatch)


@pytest.mark.parametrize("name", ["built10", "reset10", "built32", "reset32", "crowded10"])
def test_fused_wave_step_f64(monkeypatch, tdm_obs, name):  # noqa: F811
    ref = reference(tdm_obs, name)
    set_form(monkeypatch, FUSED)
    for plan in plans_for(name, 5):
        w = make_world(ref, True)
        assert flags(w) == 0
        run(ref, w, plan, fused_writer(ref["N"], True))
    clear_form(monkeypatch)


# ---- the split observation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["built2", "built10", "built32", "built64", "crowded10", "crowded16"])
def test_split_observation(monkeypatch, tdm_obs, name, f64):  # noqa: F811
    """tdm_observe_snap per step, as a trajectory of 19 (chunks of 8, 8 and 3 on two snapshot halves) and
    after an overwrite rollout."""
    ref = reference(tdm_obs, name)
    set_form(monkeypatch, SPLIT)
    if name.startswith("built"):
        plans = [[("observe", 0), ("steps", 1), ("traj", 19), ("steps", 3)], [("rollout", 20)]]
    else:
        plans = [[("steps", 21), ("traj", 19)]]
    for plan in plans:
        w = make_world(ref, f64)
        assert flags(w) == _abi.LAUNCH_SPLIT_OBS
        t = run(ref, w, plan, "split observation (tdm_observe_snap)")
    some_dead(ref, t)
    clear_form(monkeypatch)


# ---- the tail observation -----------------------------------------------------------------------------------

@pytest.mark.parametrize("workers", [None, "0"], ids=["workers-default", "workers-0"])
@pytest.mark.parametrize("K", [5, 33])
@pytest.mark.parametrize("name,f64", [("built16", False), ("built32", False), ("built10", False), ("built33", False),
                                      ("built16", True)])
def test_tail_observation(monkeypatch, tdm_obs, name, f64, K, workers):  # noqa: F811
    """tdm_tail_row: N = 16 and 32 staged with the mask in 16-byte pieces (N (N - 1) a multiple of 16), N = 10
    staged with the byte mask, N = 33 and float64 the pair tiles; K = 33 takes the balanced env order;
    observed by the observe-only blocks, or (workers 0) by the physics waves alone."""
    ref = reference(tdm_obs, name)
    env = dict(TAIL)
    if workers is not None:
        env["MACM_TDM_TAIL_WORKERS"] = workers
    set_form(monkeypatch, env)
    w = make_world(ref, f64)
    assert flags(w) == _abi.LAUNCH_TAIL_OBS
    staged = not f64 and 9 <= ref["N"] <= 32
    pieces = staged and (ref["N"] * (ref["N"] - 1)) % 16 == 0
    writer = "tail observation: " + ("rowblocks, mask pieces" if pieces else "rowblocks, byte mask" if staged else "pairs")
    t = run(ref, w, [("observe", 0), ("steps", 1), ("traj", K)], writer, fused_writer(ref["N"], f64))
    some_dead(ref, t)
    clear_form(monkeypatch)


@pytest.mark.parametrize("name", ["crowded10", "crowded16"])
def test_tail_observation_crowded(monkeypatch, tdm_obs, name):  # noqa: F811
    ref = reference(tdm_obs, name)
    set_form(monkeypatch, TAIL)
    w = make_world(ref, False)
    assert flags(w) == _abi.LAUNCH_TAIL_OBS
    t = run(ref, w, [("traj", 33), ("traj", 7)], "tail observation: rowblocks")
    some_dead(ref, t)
    clear_form(monkeypatch)


# ---- the spill step -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,f64", [("built10", False), ("crowded10", False), ("built10", True), ("built65", False)])
def test_spill_step(monkeypatch, tdm_obs, name, f64):  # noqa: F811
    """DEBUG_FORCE_SPILL: N = 10 writes with tdm_obs_pairs by thread index, N = 65 in memory order."""
    ref = reference(tdm_obs, name)
    set_form(monkeypatch, FUSED)
    N = ref["N"]
    for plan in plans_for(name, 5):
        w = make_world(ref, f64, _abi.DEBUG_FORCE_SPILL)
        t = run(ref, w, plan, "spill step: " + ("pairs" if N <= 64 else "linear"))
        assert w.spilled() > 0
    some_dead(ref, t)
    clear_form(monkeypatch)


# ---- the workgroup step (N > 64) ------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["built65", "reset65", "built130", "reset130"])
def test_workgroup_step_and_observe(monkeypatch, tdm_obs, name, f64):  # noqa: F811
    """reset() and observe() write with tdm_obs_block (pair round robin), the steps with tdm_obs_block_linear;
    observe() after the last step returns the bits that step wrote."""
    ref = reference(tdm_obs, name)
    clear_form(monkeypatch)
    w = make_world(ref, f64)
    assert flags(w) == 0
    first = [("observe", 0)] if name.startswith("built") else [("reset", 0), ("observe", 0)]
    t = run(ref, w, first + [("steps", 2), ("traj", 3), ("rollout", 2)], "workgroup step (linear) / observe (block)")
    assert w.spilled() > 0, "env-steps above 64 agents are the workgroup step's"
    stepped = (w.obs.cpu().numpy().copy(), w.mask.cpu().numpy().copy())
    w.observe()
    assert_same_mask_bytes(w.mask.cpu().numpy(), stepped[1], "observe() after the last step against that step's mask")
    assert_same_obs_bits(w.obs.cpu().numpy(), stepped[0], "observe() (block) after the last step against that step's (linear)")
    same_obs(ref, t, w.obs, w.mask, f64, "observe() (block) after the last step")


# ---- wave observe() and the observation reset() writes ----------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["built10", "reset10", "built64", "reset64"])
def test_wave_observe_and_reset(monkeypatch, tdm_obs, name, f64):  # noqa: F811
    ref = reference(tdm_obs, name)
    clear_form(monkeypatch)
    w = make_world(ref, f64)
    first = [("observe", 0)] if name.startswith("built") else [("reset", 0), ("observe", 0)]
    run(ref, w, first + [("steps", 2), ("observe", 0)], "wave reset / observe (pairs)")


# ---- a coincident alive pair: observe() only ------------------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [10, 65])
def test_coincident_pair_observed(tdm_obs, N, f64):  # noqa: F811
    """Two alive agents on one point (r = +0, t = wrap(+0 - angle)), in one block (0, 1) and across blocks
    (2, N - 1), both index orders; stepping such a pair is the physics tests' business."""
    teams, E, kw = TEAMS[N], 2, dict(world_width=30.0, world_height=30.0)
    pos, ang, alive = (a[:E].copy() for a in constructed_state(teams))
    alive[:] = 1
    pos[:, 1] = pos[:, 0]
    pos[:, N - 1] = pos[:, 2]
    orc = OracleTDM(tdm_config(teams, obs_f64=True, **kw), E, 9)
    inject_tdm(None, orc, pos, ang, alive=alive, health=alive.astype(np.float64))
    st = orc.get_state()
    o32, o64, m = tdm_obs(st["pos"], st["angle"], st["alive"], teams)
    assert m.all() and (as_bits(o64)[:, 0, 0, 0] == 0).all() and (as_bits(o64)[:, N - 1, 2, 0] == 0).all()
    w = TdmWorld(tdm_config(teams, obs_f64=f64, **kw), E, device="cuda:0")
    w.reset(9, 0)
    w.set_state(st)
    w.observe()
    ctx = "observe() of coincident pairs: " + ("wave (pairs)" if N <= 64 else "workgroup (block)")
    assert_same_mask_bytes(w.mask.cpu().numpy(), m, ctx)
    assert_same_obs_bits(w.obs.cpu().numpy(), o64 if f64 else o32, ctx)
