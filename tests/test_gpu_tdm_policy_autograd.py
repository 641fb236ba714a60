"""TdmSetPolicy.forward under torch.autograd: its logits are the bits a policy rollout stored for the policy's
agents, a torch loss's backward through it leaves params.grad within tdm_grad_ref.tol of the reference fed with
the loss's own dL/dlogits, two backwards accumulate, an optimizer step in place is seen by the next forward and
by the next rollout launch without a second registration, and `agents` leaves the other team's rows out."""
import numpy as np
import pytest
import torch

import tdm_grad_ref as tg
import tdm_policy_ref as ref

pytestmark = pytest.mark.gpu

from gym_macm.bots import combat_actions  # noqa: E402
from gym_macm.tdm_policy import HEADS, N_LOGITS, TdmSetPolicy  # noqa: E402
from gym_macm.tdm_world import TdmWorld, tdm_config  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
TEAMS, E, K, H = [4, 4], 8, 6, 32
N = sum(TEAMS)


def seeded_policy(grad=True):
    pol = TdmSetPolicy(H, DEV)
    pol.params.copy_(torch.from_numpy(ref.seeded_params(H)))
    if grad:
        pol.params.requires_grad_()
    return pol


def collect(pol, teams=(0,), dead=False):
    """One trajectory launch of K steps with the policy on `teams`: (world, traj, logits [K, E, N, 11], acts).
    dead: agent 1 of env 0 starts dead (a constructed state), so rows with an empty set and masked slots occur
    from step 0 on."""
    w = TdmWorld(tdm_config(TEAMS, world_width=8.0, world_height=8.0), E, device=DEV)
    w.reset(23)
    if dead:
        s = w.get_state()
        s["alive"][0, 1], s["health"][0, 1] = 0, 0.0
        w.set_state(s)
        w.observe()
    w.set_policy(pol, list(teams))
    acts = torch.empty((K + 1, E, N, 4), dtype=torch.uint8, device=DEV)
    combat_actions(w.obs, w.mask, out=acts[0])
    pol.act(w.obs, w.mask, w.health, out=acts[0], agents=w.policy_agents(list(teams)))
    noise = torch.from_numpy(ref.gumbel_noise((K, E, N, N_LOGITS), 5)).to(DEV)
    logits = torch.full((K, E, N, N_LOGITS), float("nan"), dtype=torch.float32, device=DEV)
    traj = w.rollout_policy_traj(acts, K, noise=noise, logits=logits)
    torch.cuda.synchronize()
    assert w.status() == 0
    return w, traj, logits, acts


def head_loss(z, actions, adv):
    """An advantage-weighted log-likelihood over the four heads of MultiDiscrete([3, 3, 3, 2])."""
    at, total = 0, 0.0
    for h, n in enumerate(HEADS):
        logp = torch.log_softmax(z[..., at:at + n], dim=-1)
        total = total - (adv * logp.gather(-1, actions[..., h:h + 1].long()).squeeze(-1)).sum()
        at += n
    return total / adv.numel()


def learner_inputs(traj, acts, seed=3):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    adv = torch.randn((K, E, N), device=DEV, generator=g)
    return traj["obs"], traj["mask"], traj["health"], acts[1:], adv


@pytest.mark.parametrize("dead", [False, True], ids=["reset", "dead_agent"])
def test_forward_has_the_rollouts_bits(dead):
    pol = seeded_policy()
    w, traj, logits, _ = collect(pol, dead=dead)
    team0 = w.policy_agents([0]).bool()
    if dead:
        m = traj["mask"][0, 0]
        assert int(m[1].sum()) == 0 and int(m[0].sum()) == N - 2, "the dead agent sees nobody and nobody sees it"
    for requires_grad in (True, False):
        pol.params.requires_grad_(requires_grad)
        z = pol.forward(traj["obs"], traj["mask"], traj["health"])
        assert z.requires_grad == requires_grad and tuple(z.shape) == (K, E, N, N_LOGITS)
        assert torch.equal(z.detach()[:, :, team0].view(torch.int32), logits[:, :, team0].view(torch.int32))
        assert not torch.isnan(logits[:, :, team0]).any() and torch.isnan(logits[:, :, ~team0]).all()


def test_backward_against_the_reference_and_accumulation():
    pol = seeded_policy()
    _, traj, _, acts = collect(pol, dead=True)
    obs, mask, health, actions, adv = learner_inputs(traj, acts)
    z = pol.forward(obs, mask, health)
    z.retain_grad()
    head_loss(z, actions, adv).backward()
    torch.cuda.synchronize()
    got = pol.params.grad.cpu().numpy().astype(F64)
    dl = z.grad.cpu().numpy()
    g, G = tg.grad(pol.params.detach().cpu().numpy(), H, obs.cpu().numpy(), mask.cpu().numpy(),
                   health.cpu().numpy(), dl)
    rows = K * E * N
    bound = tg.tol(G, rows, H)
    used = (np.abs(got - g)[G > 0] / bound[G > 0]).max()
    print(f"autograd backward, {rows} rows: {used:.4f} of the bound")
    assert np.isfinite(got).all() and np.abs(got).max() > 0 and used <= 1.0
    assert not got[G == 0].any()
    # the bits of a direct call on the same dL/dlogits, and a second backward adds to them
    direct = pol.param_grad(obs, mask, health, z.grad.contiguous())
    assert torch.equal(direct.view(torch.int32), pol.params.grad.view(torch.int32))
    head_loss(pol.forward(obs, mask, health), actions, adv).backward()
    assert torch.equal(pol.params.grad, direct + direct)
    assert list(pol._grad_ws) == [rows], "one workspace per row count"


def test_an_optimizer_step_is_seen_without_registration():
    pol = seeded_policy()
    w, traj, logits0, acts = collect(pol)
    obs, mask, health, actions, adv = learner_inputs(traj, acts)
    opt = torch.optim.SGD([pol.params], lr=0.05)
    before = pol.params.detach().clone()
    head_loss(pol.forward(obs, mask, health), actions, adv).backward()
    opt.step()
    assert not torch.equal(pol.params.detach(), before)
    # the next forward: the reference's bits for the new params
    z = pol.forward(obs, mask, health).detach()
    want = ref.logits_of(pol.params.detach().cpu().numpy(), H, obs.cpu().numpy(), mask.cpu().numpy(),
                         health.cpu().numpy())
    assert np.array_equal(z.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the next rollout launch of the world the policy was registered with before the step
    noise = torch.from_numpy(ref.gumbel_noise((K, E, N, N_LOGITS), 6)).to(DEV)
    logits = torch.full((K, E, N, N_LOGITS), float("nan"), dtype=torch.float32, device=DEV)
    acts2 = torch.empty_like(acts)
    acts2[0] = acts[K]
    traj2 = w.rollout_policy_traj(acts2, K, noise=noise, logits=logits)
    torch.cuda.synchronize()
    team0 = w.policy_agents([0]).bool()
    z2 = pol.forward(traj2["obs"], traj2["mask"], traj2["health"]).detach()
    assert torch.equal(z2[:, :, team0].view(torch.int32), logits[:, :, team0].view(torch.int32))
    old = seeded_policy(grad=False)
    assert not torch.equal(old.forward(traj2["obs"], traj2["mask"], traj2["health"])[:, :, team0], logits[:, :, team0])


def test_agents_leave_the_other_team_out():
    pol = seeded_policy()
    w, traj, logits, acts = collect(pol)
    obs, mask, health, actions, adv = learner_inputs(traj, acts)
    agents = w.policy_agents([0])
    team0 = agents.bool()
    # the other team's rows hold what no learner should read
    obs, health = obs.clone(), health.clone()
    obs[:, :, ~team0], health[:, :, ~team0] = float("nan"), float("nan")
    z = pol.forward(obs, mask, health, agents=agents)
    z.retain_grad()
    assert torch.equal(z.detach()[:, :, team0].view(torch.int32), logits[:, :, team0].view(torch.int32))
    assert not z.detach()[:, :, ~team0].any(), "zeros in the rows of the agents outside `agents`"
    head_loss(z, actions, adv).backward()
    torch.cuda.synchronize()
    got = pol.params.grad.cpu().numpy().astype(F64)
    dl = z.grad.cpu().numpy()
    assert np.abs(dl[:, :, (~team0).cpu().numpy()]).max() > 0, "the loss has a gradient there, which the launch skips"
    g, G = tg.grad(pol.params.detach().cpu().numpy(), H, obs.cpu().numpy(), mask.cpu().numpy(), health.cpu().numpy(),
                   dl, agents=agents.cpu().numpy())
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert (np.abs(got - g) <= tg.tol(G, K * E * N, H)).all()
