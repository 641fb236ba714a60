"""Every TDM launch form on a side stream, behind a backlog (tests/stream_order.py): the fused wave kernel's
calls, the split observation (its observation stream forked and joined by two event pairs per chunk; K = 19
runs chunks of 8, 8 and 3, so chunk 2 waits for chunk 0's observation before it overwrites its snapshot half),
two split rollouts back to back (the halves are reused), the tail observation, the workgroup step, and
events with autoreset and final outputs. Bit for bit against a twin on the default stream."""
import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


FUSED = {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "0"}
SPLIT = {"MACM_TDM_SPLIT_OBS": "1", "MACM_TDM_TAIL_OBS": "0"}
TAIL = {"MACM_TDM_SPLIT_OBS": "0", "MACM_TDM_TAIL_OBS": "1"}
OUT_KEYS = ("obs", "mask", "health", "alive", "done", "winner")


def use_form(monkeypatch, form):
    for k in ("MACM_TDM_TAIL_WORKERS", "MACM_TDM_TAIL_STEPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def world_outs(w, keys=OUT_KEYS):
    outs = {k: getattr(w, k) for k in keys}
    if w.hit_id is not None and "health" in keys:
        outs["hit_id"] = w.hit_id
    return outs


class Case:
    def __init__(self, E, teams, K, what, cfg=None, world=None, seed=17, check=None, warm=True, reserve=False):
        self.E, self.teams, self.N, self.K, self.what = E, teams, sum(teams), K, what
        self.cfg, self.world, self.seed, self.check, self.warm, self.reserve = dict(cfg or {}), dict(world or {}), seed, \
            check, warm, reserve

    def make(self):
        w = TdmWorld(tdm_config(self.teams, **self.cfg), self.E, device=DEV, **self.world)
        w.reset(self.seed)
        rig = getattr(self, "rig_" + self.what)(w)
        rig.n = 0
        if self.reserve:
            w.reserve(self.K)
        if self.warm:
            # buffer growth (tdm_split_buffers, the tail's snapshots and control words) happens here; on the decoy
            # inputs, so that what the library keeps of a call's inputs is not the real values
            rig.load("decoy")
            self.call(rig)
        torch.cuda.synchronize()
        assert w.status() == 0
        assert self.check is not None, "every case asserts the launch form it exists for"
        self.check(w)  # (an asserting function)
        if w.final_ends is not None:
            rig.ends0 = w.final_ends.clone()
        return rig

    def call(self, rig):
        rig.n += 1
        rig.fn(rig)

    def acts(self, lead, seed):
        real = so.tdm_actions(tuple(lead) + (self.E, self.N), seed)
        return (torch.empty_like(real), real, so.noop_like(real))

    def rig_step(self, w):
        acts = self.acts((), 3)
        r = Rig(w, {"actions": acts}, world_outs(w))
        r.fn = lambda r: w.step(acts[0])
        return r

    def rig_rollout(self, w):
        acts = self.acts((self.K,), 5)
        r = Rig(w, {"actions": acts}, world_outs(w))
        r.fn = lambda r: w.rollout(acts[0])
        return r

    def rig_rollout_traj(self, w):
        acts = self.acts((self.K,), 5)
        traj = w.trajectory_buffers(self.K)
        outs, inout, rows = {**world_outs(w), **{"traj_" + k: t for k, t in traj.items()}}, set(), {}
        if w.final_ends is not None:
            outs.update(final_obs=w.final_obs, final_mask=w.final_mask, final_length=w.final_length,
                        final_ends=w.final_ends)
            inout.add("final_ends")  # a count: the call adds to it
            ended = lambda out: out["final_ends"] > r.ends0  # the envs that ended in this call: their rows are written
            rows.update(final_obs=ended, final_mask=ended, final_length=ended)
        r = Rig(w, {"actions": acts}, outs, inout, rows)
        r.fn = lambda r: w.rollout_traj(acts[0], traj)
        return r

    def rig_rollout_bots(self, w):
        acts = self.acts((), 7)
        r = Rig(w, {"actions": acts}, {**world_outs(w), "next_actions": acts[0]}, inout={"next_actions"})
        r.fn = lambda r: w.rollout_bots(acts[0], self.K)
        return r

    def rig_rollout_bots_traj(self, w):
        buf = torch.empty((self.K + 1, self.E, self.N, 4), dtype=torch.uint8, device=DEV)
        first = so.tdm_actions((self.E, self.N), 7)
        traj = w.trajectory_buffers(self.K)
        outs = {**world_outs(w), **{"traj_" + k: t for k, t in traj.items()}, "bot_actions": buf[1:]}
        r = Rig(w, {"actions": (buf[0], first, so.noop_like(first))}, outs)
        r.fn = lambda r: w.rollout_bots_traj(buf, self.K, traj)
        return r

    def rig_reset(self, w):
        w.step(so.tdm_actions((self.E, self.N), 3))
        r = Rig(w, {}, world_outs(w, OUT_KEYS))
        r.outs.pop("hit_id", None)  # a reset never writes it
        r.fn = lambda r: w.reset(1000 + r.n)
        return r

    def rig_observe(self, w):
        w.step(so.tdm_actions((self.E, self.N), 3))
        r = Rig(w, {}, world_outs(w, OUT_KEYS))  # obs and mask by a kernel, the rest by four copies on the stream
        r.outs.pop("hit_id", None)
        r.fn = lambda r: w.observe()
        return r

    def rig_reset_envs(self, w):
        w.step(so.tdm_actions((self.E, self.N), 3))
        real = (torch.arange(self.E, device=DEV) % 3 != 1).to(torch.uint8)
        mask = (torch.empty_like(real), real, 1 - real)
        keys = ("obs", "mask", "health", "alive", "winner")
        rows = lambda _out: real.bool()
        r = Rig(w, {"env_mask": mask}, {k: getattr(w, k) for k in keys}, rows={k: rows for k in keys})
        r.fn = lambda r: w.reset_envs(mask[0])
        return r

    def run(self, plug=True, calls=1):
        return so.run_ordered(f"tdm {self.what} E{self.E} {self.teams} K{self.K} x{calls}", self.make, self.call,
                              plug=plug, calls=calls)


def fused(w):
    assert w.launch_flags() & (_abi.LAUNCH_SPLIT_OBS | _abi.LAUNCH_TAIL_OBS) == 0


def split(w):
    assert w.launch_flags() & _abi.LAUNCH_SPLIT_OBS and not w.launch_flags() & _abi.LAUNCH_TAIL_OBS


def tail(w):
    assert w.launch_flags() & _abi.LAUNCH_TAIL_OBS


@pytest.mark.parametrize("what", ["reset", "step", "rollout", "rollout_traj", "rollout_bots", "rollout_bots_traj",
                                  "reset_envs", "observe"])
def test_fused(monkeypatch, what):
    use_form(monkeypatch, FUSED)
    Case(8, [4, 4], 6, what, check=fused).run()


@pytest.mark.parametrize("what", ["step", "rollout", "rollout_traj"])
def test_split_observation(monkeypatch, what):
    use_form(monkeypatch, SPLIT)
    Case(8, [4, 4], 19, what, check=split).run()


def test_split_observation_two_calls_back_to_back(monkeypatch):
    """The second rollout's chunk 0 steps into the snapshot half that the first one's chunk 2 is observed from."""
    use_form(monkeypatch, SPLIT)
    Case(8, [4, 4], 19, "rollout_traj", check=split).run(calls=2)


def test_tail_observation(monkeypatch):
    """No plug: the observing blocks wait for the stepping waves' progress inside the launch."""
    use_form(monkeypatch, TAIL)
    Case(8, [4, 4], 19, "rollout_traj", check=tail).run(plug=False)


def test_tail_observation_first_call(monkeypatch):
    """The world's first tail rollout, on the side stream: the control words are allocated there and zeroed
    by a memset on the caller's stream ahead of the launch (the snapshots are reserved ahead, so nothing
    synchronises). No plug."""
    use_form(monkeypatch, TAIL)
    Case(8, [4, 4], 19, "rollout_traj", check=tail, warm=False, reserve=True).run(plug=False)


def workgroup(w):
    """N > 64: the workgroup step, one launch per step on the caller's stream, the observation inside it (no
    split, no tail, and TDM has no handoff: the plug may stay)."""
    assert w.N > 64
    fused(w)


@pytest.mark.parametrize("what", ["step", "rollout_traj"])
def test_workgroup_path(monkeypatch, what):
    use_form(monkeypatch, FUSED)
    Case(4, [40, 40], 3, what, check=workgroup).run()


def test_events_autoreset_and_final_outputs(monkeypatch):
    """A crowded world with a short time limit: combat events per step, episodes that end inside the launch,
    their last observations in the final outputs; hit_id and the final rows equal the twin's."""
    use_form(monkeypatch, FUSED)
    c = Case(8, [4, 4], 19, "rollout_traj", cfg=dict(world_width=8.0, world_height=8.0, time_limit=0.25),
             world=dict(autoreset=True, final_obs=True, events=True), check=fused)
    A, _ = c.run()
    assert "traj_hit_id" in A["out"] and bool((A["out"]["traj_hit_id"] >= 0).any()), "nobody was hit"
    assert int(A["out"]["traj_done"].sum()) >= c.E, "no episode ended inside the launch"
