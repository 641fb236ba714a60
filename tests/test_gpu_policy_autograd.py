"""MlpPolicy.forward / MlpCritic.forward under torch.autograd, on a small trajectory of the closed loop (4 envs
of 8 agents, the 3 aligned decisions of a 4-step launch (gym_macm.ppo.transitions), autoreset on with every
episode ending at its 2nd step): the forward has the bits the
launch stored; the backward of a PPO-shaped torch loss gives params.grad within grad_ref.tol of the reference
fed with the loss's own dL/dlogits (dL/dvalue), and the bits of a direct macm_policy_grad (macm_value_grad)
call; two backward passes accumulate; after an optimizer step the next launch reads the new params with no
second registration."""
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
E, N, K = 4, 8, 3
F32, F64 = np.float32, np.float64
SHAPES = [(32, 2), (16, 1)]


def ibits(t):
    return t.detach().contiguous().view(torch.int32)


def seeded(cls, od, H, nh, seed):
    m = cls(od, H, nh, DEV)
    rng = np.random.default_rng([seed, od, H, nh])
    m.params.copy_(torch.from_numpy((0.3 * rng.standard_normal(m.params.numel())).astype(F32)))
    return m


def collect(H, nh, seed=37):
    """One trajectory launch with the critic beside the actor; everything a learner takes from it."""
    vec = FlockVec(E, n_agents=[N], seed=seed, device=DEV, autoreset=True, time_limit=1.5 / 60.0)
    od = vec.world.OD
    pol, crit = seeded(MlpPolicy, od, H, nh, 1), seeded(MlpCritic, od, H, nh, 2)
    vec.set_policy(pol)
    vec.set_critic(crit)
    c = dict(vec=vec, pol=pol, crit=crit, od=od)
    c.update(launch(c))
    return c


def launch(c):
    """A launch of K + 1 steps and its K aligned decisions (ppo.transitions): obs, logits, adv and ret are the
    decisions' rows; acts, vals, boot and done are the launch's own rows, cut to the steps the decisions saw."""
    vec, pol, crit = c["vec"], c["pol"], c["crit"]
    L = K + 1
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
    return dict(obs=t["obs"].clone(), done=traj["done"][:K].clone(), acts=acts[:K + 1], logits=t["logits"], vals=vals[:K + 1],
                boot=boot[:K], adv=adv, ret=ret)


def ppo_loss(lg, old_logits, actions, adv, ret, v, clip=0.2):
    """The caller's torch code: log-softmax per head, ratio, clip, value loss and an entropy term."""
    lp = torch.log_softmax(lg.view(lg.shape[:-1] + (3, 3)), -1)
    old = torch.log_softmax(old_logits.view(lp.shape), -1)
    a = actions.long().unsqueeze(-1)
    logp, old_logp = lp.gather(-1, a).squeeze(-1).sum(-1), old.gather(-1, a).squeeze(-1).sum(-1)
    ratio = torch.exp(logp - old_logp)
    pg = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vloss = 0.5 * ((v - ret) ** 2).mean()
    entropy = -(lp.exp() * lp).sum((-1, -2)).mean()
    return pg + 0.5 * vloss - 0.01 * entropy


def loss_of(c, scale=1.0):
    """(loss, logits, values) on the trajectory's rows: obs row k with the action taken from it (row k + 1).
    The old logits are the stored ones moved a little, so that the ratio leaves 1 and some rows clip."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    old = c["logits"] + 0.4 * torch.randn(c["logits"].shape, device=DEV, generator=gen)
    lg, v = c["pol"].forward(c["obs"]), c["crit"].forward(c["obs"])
    if lg.requires_grad:
        lg.retain_grad()
        v.retain_grad()
    return scale * ppo_loss(lg, old, c["acts"][1:], c["adv"], c["ret"], v), lg, v


def direct(net, m, obs, dout):
    """macm_policy_grad / macm_value_grad through ctypes, with a workspace of its own"""
    L = _abi.lib()
    rows = obs.numel() // m.in_dim
    n = ctypes.c_int64()
    _abi.check(L.macm_mlp_grad_workspace(rows, ctypes.byref(n)), "macm_mlp_grad_workspace")
    ws = torch.empty((n.value,), dtype=torch.uint8, device=DEV)
    g = torch.full((m.params.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    dout = dout.contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fn = L.macm_policy_grad if net == "policy" else L.macm_value_grad
    _abi.check(fn(ctypes.byref(m.struct()), p(obs), 1 if obs.dtype == torch.float64 else 0, rows, p(dout), p(g), p(ws),
                  n.value, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "grad")
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("H,nh", SHAPES)
def test_forward_has_the_bits_the_launch_stored(H, nh):
    c = collect(H, nh)
    done = c["done"].bool()
    assert bool(done.any()) and not bool(done.all()), "some rows ended and some did not"
    for grad in (False, True):
        c["pol"].params.requires_grad_(grad)
        c["crit"].params.requires_grad_(grad)
        lg, v = c["pol"].forward(c["obs"]), c["crit"].forward(c["obs"])
        assert lg.shape == (K, E, N, 9) and v.shape == (K, E, N) and lg.dtype == v.dtype == torch.float32
        assert lg.requires_grad == grad and v.requires_grad == grad and (lg.grad_fn is not None) == grad
        assert torch.equal(ibits(lg), ibits(c["logits"])), "logits"
        assert torch.equal(ibits(v), ibits(c["vals"][1:])), "values: V of obs row k as it stands after any reset"
        keep = ~done  # boot row k is V of the obs before the reset: the same row where the env did not end
        assert torch.equal(ibits(v)[keep], ibits(c["boot"])[keep]), "boot, on the rows that did not end"
        with torch.no_grad():
            assert not c["pol"].forward(c["obs"]).requires_grad


@pytest.mark.parametrize("H,nh", SHAPES)
def test_backward_of_a_ppo_loss(H, nh):
    c = collect(H, nh)
    pol, crit, od = c["pol"], c["crit"], c["od"]
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    loss, lg, v = loss_of(c)
    loss.backward()
    torch.cuda.synchronize()
    rows = K * E * N
    obs = c["obs"].cpu().numpy().reshape(rows, od)
    for net, m, out in (("policy", pol, lg), ("critic", crit, v)):
        assert m.params.grad is not None and m.params.grad.shape == m.params.shape
        dout = out.grad
        assert dout is not None and float(dout.abs().max()) > 0
        got = m.params.grad.cpu().numpy().astype(F64)
        g, G = gr.grad(m.params.detach().cpu().numpy(), od, H, nh, gr.N_OUT[net], obs,
                       dout.cpu().numpy().reshape(rows, -1))
        bound = gr.tol(G, rows, H)
        used = np.abs(got - g)[G > 0] / bound[G > 0]
        print(f"{net} {H}x{nh}: params.grad uses {used.max():.4f} of the bound")
        assert np.isfinite(got).all() and used.max() <= 1.0, used.max()
        assert not got[G == 0].any() and np.abs(got).max() > 0
        assert torch.equal(ibits(m.params.grad), ibits(direct(net, m, c["obs"], dout))), f"{net}: a direct call's bits"
        assert torch.equal(ibits(m.params.grad), ibits(m.param_grad(c["obs"], dout.contiguous())))


def test_two_backward_passes_accumulate():
    c = collect(32, 2)
    nets = (c["pol"], c["crit"])
    for m in nets:
        m.params.requires_grad_(True)
    single = []
    for scale in (1.0, -0.37):
        for m in nets:
            m.params.grad = None
        loss_of(c, scale)[0].backward()
        single.append([m.params.grad.clone() for m in nets])
    for m in nets:
        m.params.grad = None
    loss_of(c, 1.0)[0].backward()
    loss_of(c, -0.37)[0].backward()
    for i, m in enumerate(nets):
        assert not torch.equal(ibits(single[0][i]), ibits(single[1][i]))
        assert torch.equal(ibits(m.params.grad), ibits(single[0][i] + single[1][i])), "the float32 sum of the two"


def test_optimizer_step_is_seen_by_the_next_launch():
    H, nh = 32, 2
    c = collect(H, nh)
    pol, crit, od = c["pol"], c["crit"], c["od"]
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    at = (pol.params.data_ptr(), crit.params.data_ptr())
    before = pol.params.detach().clone()
    opt = torch.optim.SGD([pol.params, crit.params], lr=0.5)
    loss_of(c)[0].backward()
    opt.step()
    assert (pol.params.data_ptr(), crit.params.data_ptr()) == at, "params keep their address"
    assert not torch.equal(ibits(pol.params), ibits(before)), "the step moved the params"
    new = launch(c)  # no second set_policy / set_critic
    obs = new["obs"].cpu().numpy()
    want = pr.logits_of(pol.params.detach().cpu().numpy(), od, H, nh, obs)
    assert pr.same_bits(new["logits"].cpu().numpy(), want).all(), "the launch read the stepped params"
    assert not pr.same_bits(new["logits"].cpu().numpy(), pr.logits_of(before.cpu().numpy(), od, H, nh, obs)).all()
    assert torch.equal(ibits(crit.forward(new["obs"])), ibits(new["vals"][1:]))


def test_pack_on_a_tensor_that_requires_grad():
    pol = MlpPolicy(4, 16, 1, DEV)
    pol.params.requires_grad_(True)
    ws, bs = gr.split_params(pr.seeded_params(4, 16, 1), 4, 16, 1, 9)
    assert pol.pack(ws, bs) is pol
    assert pol.params.requires_grad and pol.params.is_leaf and pol.params.grad_fn is None
    assert np.array_equal(pol.params.detach().cpu().numpy(), pr.seeded_params(4, 16, 1))
    layers = [torch.nn.Linear(4, 16), torch.nn.Linear(16, 1)]
    crit = MlpCritic(4, 16, 1, DEV)
    crit.params.requires_grad_(True)
    crit.load_linear_layers(layers)
    assert crit.params.requires_grad and crit.params.is_leaf
    assert torch.equal(crit.unpack()[0][0].detach().cpu(), layers[0].weight.detach().t())


def test_value_errors():
    pol, crit = MlpPolicy(4, 32, 2, DEV), MlpCritic(4, 32, 2, DEV)
    obs = torch.zeros((5, 7, 4), device=DEV)
    for m, what in ((pol, "policy"), (crit, "critic")):
        for grad in (False, True):
            m.params.requires_grad_(grad)
            with pytest.raises(ValueError, match="obs must not require grad"):
                m.forward(obs.clone().requires_grad_(True))
            with pytest.raises(ValueError, match=f"obs must be a contiguous float32/float64 tensor on the {what}'s device"):
                m.forward(obs.cpu())
            with pytest.raises(ValueError, match="obs must be a contiguous"):
                m.forward(obs.half())
            with pytest.raises(ValueError, match="obs must be a contiguous"):
                m.forward(torch.zeros((5, 7, 8), device=DEV)[..., ::2])
            with pytest.raises(ValueError, match="obs rows must have 4 values"):
                m.forward(torch.zeros((5, 7, 6), device=DEV))
        out = m.forward(obs.double())  # float64 obs are taken as stored
        assert out.shape == ((5, 7, 9) if m is pol else (5, 7)) and out.requires_grad
