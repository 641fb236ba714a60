"""gym_macm.ppo.ppo_loss under torch.autograd over MlpPolicy.forward / MlpCritic.forward on a real trajectory:
params.grad has the bits of param_grad fed with the dL/dlogits (dL/dvalue) of a direct macm_ppo_loss call and
is within grad_ref.tol of the gradient of the caller's torch loss on the same rows: evaluated in float64 on
every trajectory, and as the float32 code it is on a trajectory without saturated heads (see the test); an
outer factor reaches the kernel once, through the scale pointer; two minibatches accumulate; an Adam step is seen by the
next forward; and in the first epoch, with old_logp from log_prob on the logits rollout_policy stored, the
ratio is exactly 1."""
import ctypes

import numpy as np
import pytest
import torch

import grad_ref as gr
import policy_ref as pr

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import ppo  # noqa: E402
from gym_macm.policy import MlpCritic, MlpPolicy, gae  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SHAPES = [(32, 2), (16, 1)]


def ibits(t):
    return t.detach().contiguous().view(torch.int32)


def seeded(cls, od, H, nh, seed, sigma=0.3):
    m = cls(od, H, nh, DEV)
    rng = np.random.default_rng([seed, od, H, nh])
    m.params.copy_(torch.from_numpy((sigma * rng.standard_normal(m.params.numel())).astype(F32)))
    return m


def collect(H, nh, E=4, N=8, K=3, seed=37, sigma=0.3):
    """One trajectory launch with the critic beside the actor; everything a learner takes from it. sigma: the
    spread of the actor's seeded params (0.3: some heads' probabilities saturate on these obs rows)."""
    vec = FlockVec(E, n_agents=[N], seed=seed, device=DEV, autoreset=True, time_limit=1.5 / 60.0)
    od = vec.world.OD
    pol, crit = seeded(MlpPolicy, od, H, nh, 1, sigma), seeded(MlpCritic, od, H, nh, 2)
    vec.set_policy(pol)
    vec.set_critic(crit)
    L = K + 1  # a launch of K + 1 steps has K aligned decisions (ppo.transitions): the row counts stay K E N
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    acts = torch.empty((L + 1, E, N, 3), dtype=torch.uint8, device=DEV)
    pol.act(vec.obs, out=acts[0])
    noise = torch.from_numpy(np.concatenate([pr.gumbel_noise((K, E, N, 9), 5), pr.gumbel_noise((1, E, N, 9), 6)])).to(DEV)
    lg, vals, boot = f32(L, E, N, 9), f32(L + 1, E, N), f32(L, E, N)
    crit.value(vec.obs, out=vals[0])
    traj = vec.rollout_policy(acts, L, noise=noise, trajectory=True, logits=lg, values=vals, boot=boot)
    t = ppo.transitions(traj, acts, lg, vals, boot)
    adv, ret = gae(t["reward"], t["values"], t["boot"], t["done"], 0.99, 0.95)
    torch.cuda.synchronize()
    lg = t["logits"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    old_logits = lg + 0.4 * torch.randn(lg.shape, device=DEV, generator=gen)  # the ratio leaves 1, some rows clip
    actions = t["actions"]
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    return dict(pol=pol, crit=crit, od=od, obs=t["obs"].clone(), actions=actions, logits=lg, vals=t["values"], adv=adv,
                ret=ret, old_logits=old_logits, old_logp=ppo.log_prob(old_logits, actions), rows=K * E * N)


def torch_loss(lg, old_logp, actions, adv, ret, v, clip=0.2):
    """The caller's torch code (tools/grad_bench.py's, with old_logp given), in the dtype of its arguments"""
    lp = torch.log_softmax(lg.view(lg.shape[:-1] + (3, 3)), -1)
    a = actions.long().unsqueeze(-1)
    logp = lp.gather(-1, a).squeeze(-1).sum(-1)
    ratio = torch.exp(logp - old_logp)
    pg = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vloss = 0.5 * ((v - ret) ** 2).mean()
    entropy = -(lp.exp() * lp).sum((-1, -2)).mean()
    return pg + 0.5 * vloss - 0.01 * entropy


def direct_loss(c, lg, v, scale=None, sl=slice(None)):
    """(dlogits, dvalues, stats) of one macm_ppo_loss call through ctypes, with a workspace of its own"""
    lg, v = lg.detach()[sl].contiguous(), v.detach()[sl].contiguous()
    rows = v.numel()
    ws = torch.empty((ppo.workspace_bytes(rows),), dtype=torch.uint8, device=DEV)
    dl, dv = torch.full_like(lg, float("nan")), torch.full_like(v, float("nan"))
    stats = torch.empty((8,), dtype=torch.float64, device=DEV)
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV) if scale is not None else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cfg = ppo.config()
    _abi.check(_abi.lib().macm_ppo_loss(ctypes.byref(cfg), rows, p(lg), p(c["actions"][sl]), p(c["old_logp"][sl]),
                                        p(c["adv"][sl]), p(v), p(c["ret"][sl]), None, p(sc), p(dl), p(dv), p(stats),
                                        p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "macm_ppo_loss")
    torch.cuda.synchronize()
    return dl, dv, stats


def backward(c, factor=None, sl=slice(None)):
    """ppo.ppo_loss over the two forwards on the rows of sl, backward; returns (loss, stats, logits, values)"""
    obs = c["obs"][sl]
    lg, v = c["pol"].forward(obs), c["crit"].forward(obs)
    loss, stats = ppo.ppo_loss(lg, v, c["actions"][sl], c["old_logp"][sl], c["adv"][sl], c["ret"][sl])
    (loss if factor is None else factor * loss).backward()
    return loss, stats, lg, v


def clear(c):
    c["pol"].params.grad = c["crit"].params.grad = None


SATURATED = 1 - 1e-4  # a head counts as saturated where its largest probability is above this


@pytest.mark.parametrize("sigma", [0.3, 0.1])
@pytest.mark.parametrize("H,nh", SHAPES)
def test_backward_has_the_bits_of_a_direct_call_and_is_close_to_the_torch_loss(H, nh, sigma):
    c = collect(H, nh, sigma=sigma)
    top = torch.softmax(c["logits"].view(-1, 3, 3), -1).amax(-1)
    saturated = float((top > SATURATED).float().mean())
    print(f"{H}x{nh} sigma {sigma}: max |logit| {float(c['logits'].abs().max()):.2f}, {saturated:.3f} of the heads saturated")
    if sigma == 0.1:
        assert saturated == 0.0, "the condition of the float32 comparison below"
    pol, crit, od, rows = c["pol"], c["crit"], c["od"], c["rows"]
    loss, stats, lg, v = backward(c)
    assert loss.dtype == torch.float32 and loss.shape == () and loss.requires_grad
    assert stats.dtype == torch.float64 and stats.shape == (8,) and not stats.requires_grad
    dl, dv, dstats = direct_loss(c, lg, v)
    assert torch.equal(stats.view(torch.int64), dstats.view(torch.int64))
    assert float(loss.detach()) == float(np.float32(stats[0].item())) and 0 < float(stats[5]) < 1 and float(stats[7]) == rows
    mine = {}
    for net, m, dout in (("policy", pol, dl), ("critic", crit, dv)):
        assert torch.equal(ibits(m.params.grad), ibits(m.param_grad(c["obs"], dout))), net
        mine[net] = m.params.grad.cpu().numpy().astype(F64)
    obs = c["obs"].cpu().numpy().reshape(rows, od)
    # The torch loss on the same float32 logits and values, evaluated in float64 and in float32 (the caller's
    # code as it stands). Against float64 the bound holds on every trajectory. Against float32 it is asserted
    # where no head is saturated (sigma = 0.1): float32 autograd forms dL/dlogit of a taken action as g - p g,
    # which loses g (1 - p) to cancellation where p is within a few float32 ulps of 1, so on a trajectory with
    # such heads (sigma = 0.3 on these obs rows) its own error is not small against |dL/dlogits|, which is what
    # grad_ref's magnitude G is built from. There the float32 figure is printed only.
    for dt in (torch.float64, torch.float32):
        clear(c)
        lg, v = pol.forward(c["obs"]), crit.forward(c["obs"])
        lg.retain_grad()
        v.retain_grad()
        torch_loss(lg.to(dt), c["old_logp"].to(dt), c["actions"], c["adv"].to(dt), c["ret"].to(dt), v.to(dt)).backward()
        for net, m, out in (("policy", pol, lg), ("critic", crit, v)):
            _, G = gr.grad(m.params.detach().cpu().numpy(), od, H, nh, gr.N_OUT[net], obs,
                           out.grad.cpu().numpy().reshape(rows, -1))
            bound = gr.tol(G, rows, H)
            err = np.abs(mine[net] - m.params.grad.cpu().numpy().astype(F64))
            print(f"{net} {H}x{nh}: {(err[G > 0] / bound[G > 0]).max():.4f} of the bound from the gradient of the "
                  f"torch loss in {dt}")
            if dt == torch.float64 or sigma == 0.1:
                assert np.all(err <= bound) and np.abs(mine[net]).max() > 0


def test_an_outer_factor_reaches_the_kernel_once():
    c = collect(32, 2)
    backward(c)
    full = [m.params.grad.clone() for m in (c["pol"], c["crit"])]
    clear(c)
    _, _, lg, v = backward(c, factor=0.5)
    dl, dv, _ = direct_loss(c, lg, v, scale=0.5)
    for m, dout, f in ((c["pol"], dl, full[0]), (c["crit"], dv, full[1])):
        assert torch.equal(ibits(m.params.grad), ibits(m.param_grad(c["obs"], dout)))
        assert torch.allclose(2 * m.params.grad, f, rtol=1e-6, atol=0), "half of the full gradient, not a quarter"


def test_two_minibatches_accumulate():
    c = collect(32, 2)
    nets = (c["pol"], c["crit"])
    single = []
    for sl in (slice(0, 2), slice(2, 3)):  # contiguous slices of the leading dimension
        clear(c)
        backward(c, sl=sl)
        single.append([m.params.grad.clone() for m in nets])
    clear(c)
    backward(c, sl=slice(0, 2))
    backward(c, sl=slice(2, 3))
    for i, m in enumerate(nets):
        assert not torch.equal(ibits(single[0][i]), ibits(single[1][i]))
        assert torch.equal(ibits(m.params.grad), ibits(single[0][i] + single[1][i])), "the float32 sum of the two"


def test_an_adam_step_is_seen_by_the_next_forward():
    H, nh = 32, 2
    c = collect(H, nh)
    pol, crit, od = c["pol"], c["crit"], c["od"]
    before = pol.params.detach().clone()
    at = (pol.params.data_ptr(), crit.params.data_ptr())
    opt = torch.optim.Adam([pol.params, crit.params], lr=1e-2)
    backward(c)
    opt.step()
    assert (pol.params.data_ptr(), crit.params.data_ptr()) == at, "params keep their address"
    assert not torch.equal(ibits(pol.params), ibits(before)), "the step moved the params"
    lg = pol.forward(c["obs"])
    obs = c["obs"].cpu().numpy()
    assert pr.same_bits(lg.detach().cpu().numpy(), pr.logits_of(pol.params.detach().cpu().numpy(), od, H, nh, obs)).all()
    assert not torch.equal(ibits(lg), ibits(c["logits"]))


def test_first_epoch_ratio_is_exactly_one():
    c = collect(32, 2, E=2, N=3, K=4)
    old_logp = ppo.log_prob(c["logits"], c["actions"])  # from the logits rollout_policy stored
    lg, v = c["pol"].forward(c["obs"]), c["crit"].forward(c["obs"])
    assert torch.equal(ibits(lg), ibits(c["logits"]))
    loss, stats = ppo.ppo_loss(lg, v, c["actions"], old_logp, c["adv"], c["ret"])
    s = stats.cpu().numpy()
    assert s[4] == 0.0 and s[5] == 0.0 and s[6] == 1.0 and s[7] == 2 * 3 * 4, s
    loss.backward()
    assert float(c["pol"].params.grad.abs().max()) > 0 and bool(torch.isfinite(c["pol"].params.grad).all())
