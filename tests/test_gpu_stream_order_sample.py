"""The sampled launches on a side stream, behind a backlog (tests/stream_order.py): the policy rollout of a
world with sampling on (wave path with autoreset and final outputs, and the workgroup path's loop), and both
one-shot kernels, macm_policy_noise and macm_policy_flock_sampled. Each case compares the side-stream run
with a twin on the default stream bit for bit. The draw itself has no device input to write late (seed and
decision travel by value); the obs, the first actions and both nets' params are written late as before."""
import pytest
import torch

import stream_order as so
from stream_order import DEV, Rig
from test_gpu_stream_order_flock import SHORT, Case, floats, is_wave, plain_wg, world_outs
from test_gpu_stream_order_learn import late_floats, nets, run

pytestmark = pytest.mark.gpu

from gym_macm.policy import MlpCritic, MlpPolicy, gumbel_noise  # noqa: E402

SEED = 0x0BAD_5EED_0123_4567


@pytest.fixture(scope="module", autouse=True)
def _controls_hold():
    so.require_controls()


class SampleCase(Case):
    def rig_policy_sampled(self, v):
        """Case.rig_policy on a world with sampling on: no noise input. The warm-up call advances the world's
        decision by K on every instance alike."""
        K, E, N, od = self.K, self.E, self.N, v.obs_dim
        pol, crit = MlpPolicy(od, 16, 2, device=DEV), MlpCritic(od, 32, 1, device=DEV)
        v.set_policy(pol)
        v.set_critic(crit)
        v.set_sampling(SEED, 2**32 - 2)
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        vals = torch.empty((K + 1, E, N), dtype=torch.float32, device=DEV)
        first = so.flock_actions((E, N), 7)
        ins = {"actions": (acts[0], first, so.noop_like(first)),
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

        def fn(r):
            d = v.sampling[1]
            v.rollout_policy(acts, K, trajectory=True, traj=traj, logits=logits, values=vals, boot=boot)
            assert v.sampling == (SEED, d + K)
        r.fn = fn
        return r


def test_sampled_rollout_wave():
    c = SampleCase(8, 16, 6, "policy_sampled", dict(autoreset=True, final_obs=True, time_limit=SHORT), check=is_wave)
    A, _ = c.run()
    assert int(A["out"]["traj_done"].sum()) >= 8, "every env ends inside the launch"
    assert len(torch.unique(A["out"]["acts"])) == 3


def test_sampled_rollout_workgroup_loop(monkeypatch):
    """The loop's launches in plain order (the handoff has its own case in test_gpu_stream_order_flock.py)."""
    monkeypatch.setenv("MACM_HANDOFF", "0")
    SampleCase(2, 96, 3, "policy_sampled", dict(start_spread=12), check=plain_wg).run()


@pytest.mark.parametrize("rows", (65, 4097))
def test_policy_act_sampled(rows):
    def build():
        pol, _ = nets()
        ins = {"obs": late_floats((rows, 4), 3),
               "params": (pol.params, floats(pol.params.shape, 7, 0.7), floats(pol.params.shape, 8, 0.7))}
        outs = {"actions": torch.empty((rows, 3), dtype=torch.uint8, device=DEV),
                "logits": torch.empty((rows, 9), dtype=torch.float32, device=DEV)}
        r = Rig(None, ins, outs)
        r.fn = lambda r: pol.act(ins["obs"][0], seed=SEED, decision=9, logits=outs["logits"], out=outs["actions"])
        return r
    run(f"policy.act sampled {rows}", build)


@pytest.mark.parametrize("rows", (65, 4097))
def test_gumbel_noise(rows):
    """No device input: the outputs are allocated inside the call, over a block that held the prefill."""
    def build():
        r = Rig(None, {}, {})

        def fn(r):
            so.poison((3, rows, 9), torch.float32)
            r.outs["noise"], r.outs["words"] = gumbel_noise(SEED, 2**32 - 1, 3, (rows,), DEV, words=True)
        r.fn = fn
        return r
    run(f"gumbel_noise {rows}", build)
