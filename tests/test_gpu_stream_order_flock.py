"""Every Flock launch path on a side stream, behind a backlog (tests/stream_order.py): the wave kernel's
calls in both observation forms, autoreset with final outputs, the forced spill step, the workgroup path in
plain launch order, with the B -> C handoff and over env slices on streams of their own, the step above 1024
agents, the learned policy and critic inside the launch, and set_state followed by a step. Each case
compares the side-stream run with a twin on the default stream bit for bit: outputs, state, counters, reward
sums; status 0 on both."""
import numpy as np
import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


# time_limit: an episode ends at its 5th step (60 Hz). The warm-up launch of 6 steps leaves every env one step
# into its second episode; the measured launch ends that one at its 4th step and is two steps into the third
# when it returns, so every env ends inside the launch and the state it leaves still depends on the actions
SHORT = 4.5 / 60.0


def world_outs(vec, keys=("obs", "nbr_id", "reward", "collided", "done")):
    return {k: getattr(vec.world, k) for k in keys}


def late(real, decoy=None):
    """(buf, real, decoy) of one input: the buffer the call reads, and its two staged contents."""
    decoy = so.noop_like(real) if decoy is None else decoy
    return (torch.empty_like(real), real, decoy)


def floats(shape, seed, scale=1.0):
    return (torch.rand(tuple(shape), device=DEV, generator=so.generator(seed)) * 2 - 1) * scale


class Case:
    """A world's configuration and one kind of call; make() builds a warmed Rig (the call made once on the
    default stream, which takes every first-call decision of the library), run() is the harness's run."""

    def __init__(self, E, N, K, what, kw=None, debug=0, seed=11, check=None):
        self.E, self.N, self.K, self.what, self.kw, self.debug, self.seed = E, N, K, what, dict(kw or {}), debug, seed
        self.check = check

    def vec(self):
        v = FlockVec(self.E, n_agents=[self.N], seed=self.seed, device=DEV, **self.kw)
        if self.debug:
            v.world.set_debug(self.debug)
        return v

    def make(self):
        v = self.vec()
        rig = getattr(self, "rig_" + self.what)(v)
        rig.n = 0
        # warm-up: the handoff decision, the slice streams, any buffer that grows on demand. On the decoy inputs,
        # so that what the library keeps of a call's inputs (the reset mask's private copy) is not the real values
        rig.load("decoy")
        self.call(rig)
        torch.cuda.synchronize()
        assert v.status() == 0
        assert self.check is not None, "every case asserts the launch form it exists for"
        self.check(v.world)  # (an asserting function)
        return rig

    def call(self, rig):
        rig.n += 1
        rig.fn(rig)

    # -- the calls ----------------------------------------------------------------------------------------
    def _cont(self):
        return self.kw.get("action_mode") == "continuous"

    def rig_step(self, v):
        acts = late(so.flock_actions((self.E, self.N), 3, self._cont()))
        r = Rig(v, {"actions": acts}, world_outs(v))
        r.fn = lambda r: v.step(acts[0])
        return r

    def rig_step_that_ends(self, v):
        """The step that ends every env's episode (SHORT: the 5th), with autoreset: the reset's launches and
        copies follow the step's on the stream. The state it leaves is the new episode's, whatever the actions."""
        for k in range(3):
            v.step(so.flock_actions((self.E, self.N), 50 + k))  # the warm-up call is the 4th step
        acts = late(so.flock_actions((self.E, self.N), 3))
        outs, inout = world_outs(v), set()
        self._final(v, outs, inout)
        r = Rig(v, {"actions": acts}, outs, inout, keep=("state",))
        r.fn = lambda r: v.step(acts[0])
        return r

    def rig_rollout(self, v):
        acts = late(so.flock_actions((self.K, self.E, self.N), 5, self._cont()))
        r = Rig(v, {"actions": acts}, world_outs(v))
        r.fn = lambda r: v.rollout(acts[0])
        return r

    def _final(self, v, outs, inout):
        if v.final_obs is not None:  # every env ends inside the launch (SHORT), so every row is written
            outs.update(final_obs=v.final_obs, final_nbr_id=v.final_nbr_id, final_length=v.final_length,
                        final_ends=v.final_ends)
            inout.add("final_ends")  # a count: the call adds to it

    def rig_rollout_traj(self, v):
        acts = late(so.flock_actions((self.K, self.E, self.N), 5, self._cont()))
        traj = v.world.trajectory_buffers(self.K)
        outs, inout = {**world_outs(v), **{"traj_" + k: t for k, t in traj.items()}}, set()
        self._final(v, outs, inout)
        r = Rig(v, {"actions": acts}, outs, inout)
        r.fn = lambda r: v.rollout(acts[0], trajectory=True, traj=traj)
        return r

    def rig_rollout_bots(self, v):
        acts = late(so.flock_actions((self.E, self.N), 7))
        r = Rig(v, {"actions": acts}, {**world_outs(v), "next_actions": acts[0]}, inout={"next_actions"})
        r.fn = lambda r: v.rollout_bots(acts[0], self.K)
        return r

    def rig_rollout_bots_traj(self, v):
        buf = torch.empty((self.K + 1, self.E, self.N, 3), dtype=torch.uint8, device=DEV)
        first = so.flock_actions((self.E, self.N), 7)
        traj = v.world.trajectory_buffers(self.K)
        outs = {**world_outs(v), **{"traj_" + k: t for k, t in traj.items()}, "bot_actions": buf[1:]}
        r = Rig(v, {"actions": (buf[0], first, so.noop_like(first))}, outs)
        r.fn = lambda r: v.rollout_bots(buf, self.K, trajectory=True, traj=traj)
        return r

    def rig_observe(self, v):
        r = Rig(v, {}, world_outs(v, ("obs", "nbr_id")))
        r.fn = lambda r: v.observe()
        return r

    def rig_reset(self, v):
        v.step(so.flock_actions((self.E, self.N), 3, self._cont()))  # away from a fresh world
        r = Rig(v, {}, world_outs(v, ("obs", "nbr_id", "done")))
        r.fn = lambda r: v.reset(1000 + r.n)  # another seed at every call: the state must change
        return r

    def rig_reset_envs(self, v):
        v.step(so.flock_actions((self.E, self.N), 3, self._cont()))
        real = (torch.arange(self.E, device=DEV) % 3 != 1).to(torch.uint8)  # both values occur
        mask = (torch.empty_like(real), real, 1 - real)
        rows = lambda _t: real.bool()
        r = Rig(v, {"mask": mask}, world_outs(v, ("obs", "nbr_id")), rows={"obs": rows, "nbr_id": rows})
        r.fn = lambda r: v.reset_envs(mask[0])
        return r

    def rig_policy(self, v):
        K, E, N, od = self.K, self.E, self.N, v.obs_dim
        pol, crit = MlpPolicy(od, 16, 2, device=DEV), MlpCritic(od, 32, 1, device=DEV)
        v.set_policy(pol)
        v.set_critic(crit)
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        vals = torch.empty((K + 1, E, N), dtype=torch.float32, device=DEV)
        first = so.flock_actions((E, N), 7)
        ins = {"actions": (acts[0], first, so.noop_like(first)),
               "noise": late(floats((K, E, N, 9), 21, 2.0), floats((K, E, N, 9), 22, 2.0)),
               "values0": (vals[0], floats((E, N), 23), floats((E, N), 24)),
               "policy_params": (pol.params, floats(pol.params.shape, 25, 0.7), floats(pol.params.shape, 26, 0.7)),
               "critic_params": (crit.params, floats(crit.params.shape, 27, 0.7), floats(crit.params.shape, 28, 0.7))}
        logits = torch.empty((K, E, N, 9), dtype=torch.float32, device=DEV)
        boot = torch.empty((K, E, N), dtype=torch.float32, device=DEV)
        traj = v.world.trajectory_buffers(K)
        outs = {**world_outs(v), **{"traj_" + k: t for k, t in traj.items()}, "acts": acts[1:], "logits": logits,
                "values": vals[1:], "boot": boot}
        inout = set()
        self._final(v, outs, inout)
        r = Rig(v, ins, outs, inout)
        r.fn = lambda r: v.rollout_policy(acts, K, noise=ins["noise"][0], trajectory=True, traj=traj, logits=logits,
                                          values=vals, boot=boot)
        r.nets = (pol, crit)
        return r

    def run(self, plug=True, pre=None):
        return so.run_ordered(f"flock {self.what} E{self.E} N{self.N} K{self.K} {self.kw}", self.make, self.call,
                              plug=plug, pre=pre)


def is_wave(w):
    assert w.launch_flags() == 0 and w.rollout_slices() == 0 and not w.uses_handoff() and w.N <= 64


WAVE_KW = {"polar_f32": {}, "cartesian_f64": {"coord": "cartesian", "obs_dtype": torch.float64}}


@pytest.mark.parametrize("what", ["reset", "step", "rollout", "rollout_traj", "rollout_bots", "rollout_bots_traj",
                                  "observe", "reset_envs"])
@pytest.mark.parametrize("form", list(WAVE_KW))
def test_wave(form, what):
    Case(8, 16, 6, what, WAVE_KW[form], check=is_wave).run()


def test_wave_autoreset_and_final_outputs():
    """Envs end inside the launch: the in-launch reset's draws and the final outputs are the launch's own."""
    c = Case(8, 16, 6, "rollout_traj", dict(autoreset=True, final_obs=True, time_limit=SHORT), check=is_wave)
    A, _ = c.run()
    assert int(A["out"]["traj_done"].sum()) == c.E and bool((A["out"]["final_length"] == 5).all())


def test_wave_step_with_autoreset():
    """Not a rollout: the per-step call, whose autoreset is a copy of the done flags and three more launches."""
    c = Case(8, 16, 1, "step_that_ends", dict(autoreset=True, final_obs=True, time_limit=SHORT), check=is_wave)
    A, _ = c.run()
    assert bool((A["out"]["done"] == 1).all()) and bool((A["out"]["final_length"] == 5).all())


@pytest.mark.parametrize("what", ["step", "rollout"])
def test_wave_forced_spill(what):
    c = Case(4, 32, 3, what, debug=_abi.DEBUG_FORCE_SPILL, check=is_wave)
    rigs = []
    make = c.make
    c.make = lambda: rigs.append(make()) or rigs[-1]
    c.run()
    assert all(r.obj.spilled() > 0 for r in rigs), "no env took the spill step"


def plain_wg(w):
    assert not w.uses_handoff() and w.rollout_slices() == 0 and 64 < w.N <= 1024


@pytest.mark.parametrize("what", ["step", "rollout", "rollout_traj", "rollout_bots"])
def test_workgroup_plain_order(monkeypatch, what):
    monkeypatch.setenv("MACM_HANDOFF", "0")
    Case(8, 100, 3, what, check=plain_wg).run()


def with_handoff(w):
    assert w.uses_handoff() and w.rollout_slices() == 0


@pytest.mark.parametrize("what", ["step", "rollout"])
def test_workgroup_handoff(monkeypatch, what):
    """Kernel C on the handoff's stream behind the watcher: forked from the caller's stream at the event
    before kernel B, joined back by the event behind C. No plug: the watcher waits for kernel B's progress."""
    monkeypatch.setenv("MACM_HANDOFF", "1")
    Case(8, 100, 3, what, check=with_handoff).run(plug=False)


def sliced(w):
    assert w.rollout_slices() >= 2 and not w.uses_handoff()  # (the slices run without the handoff: the plug may stay)


@pytest.mark.parametrize("what", ["rollout", "rollout_traj", "rollout_bots"])
def test_workgroup_env_slices(what):
    """The slice streams wait for an event on the caller's stream (the fork: late inputs, the backlog) and
    the caller's stream waits for each slice's last event (the join: the consumer, the late overwrite)."""
    Case(1024, 65, 3, what, check=sliced).run()


def big(w):
    assert w.N > 1024 and not w.uses_handoff() and w.rollout_slices() == 0 and w.launch_flags() == 0


@pytest.mark.parametrize("what", ["step", "rollout"])
def test_above_1024_agents(what):
    Case(2, 1025, 2, what, check=big).run()


def test_learned_policy_and_critic():
    """rollout_policy's trajectory form with logits, values and boot; the policy's and the critic's params are
    written late as well (the library reads them at the launch, on the stream)."""
    c = Case(8, 16, 6, "policy", dict(autoreset=True, final_obs=True, time_limit=SHORT), check=is_wave)
    A, _ = c.run()
    assert int(A["out"]["traj_done"].sum()) == c.E


def test_set_state_then_step():
    """set_state takes host arrays and synchronises the stream itself (twice), so it waits out any backlog
    ahead of it: on the side stream it shows only that it touches neither stream 0 (the plug holds that) nor
    the state after it returns. The harness therefore queues a second backlog behind it, and the step runs
    behind that one with late actions, on the state set_state injected, with no synchronisation between."""
    E, N = 4, 16
    src = FlockVec(E, n_agents=[N], seed=99, device=DEV)
    for k in range(3):
        src.step(so.flock_actions((E, N), 40 + k))
    state = src.get_state()
    c = Case(E, N, 1, "step", check=is_wave)
    A, _ = c.run(pre=lambda rig: rig.obj.set_state(state))
    # the step started from the injected state, not from the world's own
    src.step(so.flock_actions((E, N), 3))  # rig_step's real actions
    np.testing.assert_array_equal(A["state"]["pos"], src.get_state()["pos"])
