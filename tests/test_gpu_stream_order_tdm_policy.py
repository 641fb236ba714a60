"""The TDM policy launches on a side stream, behind a backlog (tests/stream_order.py): both forms of
macm_tdm_rollout_policy on the wave path, with autoreset, events and final outputs, on the workgroup path
(the launches of the step, the bots kernel and macm_policy_tdm, all on the caller's stream), and the
one-shot macm_policy_tdm. Bit for bit against a twin on the default stream."""
import pytest
import torch

import stream_order as so
import tdm_policy_ref as ref
from stream_order import DEV, Rig

pytestmark = pytest.mark.gpu

from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.tdm_policy import TdmSetPolicy  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402

NL = ref.N_LOGITS
OUT_KEYS = ("obs", "mask", "health", "alive", "done", "winner")


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


def seeded_policy(H=32):
    pol = TdmSetPolicy(H, DEV)
    pol.params.copy_(torch.from_numpy(ref.seeded_params(H)))
    return pol


def noise_pair(shape, seed):
    """(buf, real, decoy): Gumbel noise, and zeros (the argmax) as its decoy"""
    real = torch.from_numpy(ref.gumbel_noise(shape, seed)).to(DEV)
    return (torch.empty_like(real), real, torch.zeros_like(real))


class Case:
    def __init__(self, E, teams, K, what, pol_teams=None, cfg=None, world=None, seed=17):
        self.E, self.teams, self.N, self.K, self.what, self.pol_teams = E, teams, sum(teams), K, what, pol_teams
        self.cfg, self.world, self.seed = dict(cfg or {}), dict(world or {}), seed

    def make(self):
        w = TdmWorld(tdm_config(self.teams, **self.cfg), self.E, device=DEV, **self.world)
        w.reset(self.seed)
        w.set_policy(seeded_policy(), self.pol_teams)
        rig = getattr(self, "rig_" + self.what)(w)
        rig.n = 0
        rig.load("decoy")  # the warm-up call, on the decoy inputs
        self.call(rig)
        torch.cuda.synchronize()
        assert w.status() == 0
        if w.final_ends is not None:
            rig.ends0 = w.final_ends.clone()
        return rig

    def call(self, rig):
        rig.n += 1
        rig.fn(rig)

    def first(self, w):
        real = combat_actions(w.obs, w.mask)
        w.policy.act(w.obs, w.mask, w.health, out=real, agents=w.policy_agents(self.pol_teams))
        return real

    def world_outs(self, w):
        outs = {k: getattr(w, k) for k in OUT_KEYS}
        if w.hit_id is not None:
            outs["hit_id"] = w.hit_id
        return outs

    def rig_rollout_policy(self, w):
        E, N, K = self.E, self.N, self.K
        real = self.first(w)
        acts = (torch.empty_like(real), real, so.noop_like(real))
        noise = noise_pair((K, E, N, NL), 5)
        outs = {**self.world_outs(w), "next_actions": acts[0]}
        if self.pol_teams is None:  # (a bot-driven agent's logits row is not written: every team, then)
            outs["logits"] = torch.empty((E, N, NL), dtype=torch.float32, device=DEV)
        r = Rig(w, {"actions": acts, "noise": noise}, outs, inout={"next_actions"})
        r.fn = lambda r: w.rollout_policy(acts[0], K, noise=noise[0], logits=outs.get("logits"))
        return r

    def rig_rollout_policy_traj(self, w):
        E, N, K = self.E, self.N, self.K
        buf = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
        first = self.first(w)
        noise = noise_pair((K, E, N, NL), 5)
        traj = w.trajectory_buffers(K)
        outs = {**self.world_outs(w), **{"traj_" + k: t for k, t in traj.items()}, "actor_actions": buf[1:]}
        inout, rows = set(), {}
        if self.pol_teams is None:
            outs["logits"] = torch.empty((K, E, N, NL), dtype=torch.float32, device=DEV)
        if w.final_ends is not None:
            outs.update(final_obs=w.final_obs, final_mask=w.final_mask, final_length=w.final_length,
                        final_ends=w.final_ends)
            inout.add("final_ends")
            ended = lambda out: out["final_ends"] > r.ends0
            rows.update(final_obs=ended, final_mask=ended, final_length=ended)
        r = Rig(w, {"actions": (buf[0], first, so.noop_like(first)), "noise": noise}, outs, inout, rows)
        r.fn = lambda r: w.rollout_policy_traj(buf, K, traj, noise=noise[0], logits=outs.get("logits"))
        return r

    def run(self, plug=True, calls=1):
        return so.run_ordered(f"tdm {self.what} E{self.E} {self.teams} K{self.K} teams {self.pol_teams}", self.make,
                              self.call, plug=plug, calls=calls)


@pytest.mark.parametrize("pol_teams", [None, [0]], ids=["all", "team0"])
@pytest.mark.parametrize("what", ["rollout_policy", "rollout_policy_traj"])
def test_wave_path(what, pol_teams):
    Case(8, [4, 4], 6, what, pol_teams).run()


def test_wave_path_events_autoreset_and_final_outputs():
    c = Case(8, [4, 4], 19, "rollout_policy_traj", [0], cfg=dict(world_width=8.0, world_height=8.0, time_limit=0.25),
             world=dict(autoreset=True, final_obs=True, events=True))
    A, _ = c.run()
    assert "traj_hit_id" in A["out"]
    assert int(A["out"]["traj_done"].sum()) >= c.E, "no episode ended inside the launch"


@pytest.mark.parametrize("what,pol_teams", [("rollout_policy", [1]), ("rollout_policy_traj", None)])
def test_workgroup_path(what, pol_teams):
    Case(3, [40, 40], 3, what, pol_teams).run()


def test_one_shot():
    E, N, H = 9, 33, 32
    pol = seeded_policy(H)
    g = so.generator(3)
    obs_r = torch.randn((E, N, N - 1, 4), device=DEV, generator=g) * 5
    mask_r = (torch.rand((E, N, N - 1), device=DEV, generator=g) < 0.6).to(torch.uint8)
    health_r = torch.rand((E, N), device=DEV, generator=g, dtype=torch.float64)

    def make():
        obs = (torch.empty_like(obs_r), obs_r, torch.zeros_like(obs_r))
        mask = (torch.empty_like(mask_r), mask_r, 1 - mask_r)
        health = (torch.empty_like(health_r), health_r, torch.zeros_like(health_r))
        noise = noise_pair((E, N, NL), 7)
        outs = dict(actions=torch.empty((E, N, 4), dtype=torch.uint8, device=DEV),
                    logits=torch.empty((E, N, NL), dtype=torch.float32, device=DEV))
        r = Rig(None, dict(obs=obs, mask=mask, health=health, noise=noise), outs)
        r.fn = lambda r: pol.act(obs[0], mask[0], health[0], noise=noise[0], logits=outs["logits"], out=outs["actions"])
        return r

    so.run_ordered("macm_policy_tdm", make, lambda rig: rig.fn(rig))
