"""gym_macm.ppo.update (macm_ppo_update: moments -> fused gradients -> step for every minibatch, one call)
against a twin driven by the Python loop adv_moments -> ppo_grads(index=, adv_norm=) -> Adam.step(stats) ->
zero_grad: the params, the optimiser state and the [n_mb, 8] stats bit for bit. The sources are
test_gpu_ppo_minibatch.py's 5,000 rows between poison; two epochs of ppo.minibatches(5000, 4); the smallest and
the largest net pair, float32 and float64 obs; with and without old_values, with and without normalize_adv,
either net alone, an empty minibatch in the list, and a target_kl that stops the optimiser inside the call.
The params, the state and the stats of the side under test sit between guard bands. After update the one-shot
kernels and a rollout launch read the new params with no re-registration, and Adam.step() after
ppo_loss(...).backward() has the bits of step() after ppo_grads."""
import ctypes

import numpy as np
import pytest
import torch

import ppo_ref as R
from guard_bands import Guarded
from test_gpu_ppo_minibatch import DEV, N_SRC, padded, source

pytestmark = pytest.mark.gpu

from gym_macm import ppo  # noqa: E402
from gym_macm.vec import FlockVec  # noqa: E402

HYPER = dict(lr=1e-2, max_grad_norm=0.5)  # the clip is active on some minibatches and not on others


def guarded_net(like):
    """A net of like's shape and values whose params sit between guard bands"""
    net = type(like)(like.in_dim, like.hidden, like.n_hidden, DEV)
    g = Guarded(tuple(like.params.shape), torch.float32, DEV)
    g.t.copy_(like.params.detach())
    net.params, net._guard = g.t, g
    net._struct = net.STRUCT(net.in_dim, net.hidden, net.n_hidden, 0, ctypes.c_void_p(g.t.data_ptr()))
    return net


def plain_net(like):
    net = type(like)(like.in_dim, like.hidden, like.n_hidden, DEV)
    net.params.copy_(like.params.detach())
    return net


def optimiser(src, pol=True, crit=True, guarded=False, **kw):
    make = guarded_net if guarded else plain_net
    opt = ppo.Adam(make(src["pol"]) if pol else None, make(src["crit"]) if crit else None, **dict(HYPER, **kw))
    if guarded:
        g = Guarded((opt.state.numel(),), torch.uint8, DEV)
        g.t.zero_()
        opt.state, opt._guard = g.t, g
    return opt


def epochs(n_epochs=2, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [mb for _ in range(n_epochs) for mb in ppo.minibatches(N_SRC, 4, generator=g, device=DEV)]


def rows_of(src, old_values):
    args = (src["obs"], src["actions"], src["old_logp"], src["adv"], src["ret"])
    return args, (dict(old_values=src["old_values"], vf_clip=R.VF_CLIP) if old_values else {})


def loop(opt, src, mbs, old_values=True, normalize=True):
    """The twin: the README loop with ppo.Adam.step, one minibatch at a time"""
    args, kw = rows_of(src, old_values)
    out = []
    for mb in mbs:
        if mb.numel() == 0:  # update skips it whole: a zero stats row and no step
            out.append(torch.zeros(8, dtype=torch.float64, device=DEV))
            continue
        norm = ppo.adv_moments(src["adv"], mb) if normalize and opt.pol is not None else None
        stats = ppo.ppo_grads(opt.pol, opt.crit, *args, index=mb, adv_norm=norm, **kw)
        opt.step(stats)
        opt.zero_grad()
        out.append(stats)
    torch.cuda.synchronize()
    return torch.stack(out)


def updated(opt, src, mbs, old_values=True, normalize=True):
    """ppo.update into guarded stats, the bands of everything checked"""
    args, kw = rows_of(src, old_values)
    stats = Guarded((len(mbs), 8), torch.float64, DEV)
    torch.cuda.synchronize()
    got = ppo.update(opt, *args, minibatches=mbs, normalize_adv=normalize, out=stats.t, **kw)
    torch.cuda.synchronize()
    assert got is stats.t and stats.bands_intact(), "a store outside stats"
    assert opt._guard.bands_intact(), "a store outside the optimiser's state"
    for net in (opt.pol, opt.crit):
        assert net is None or (net._guard.bands_intact() and net.params.grad is None), "a store outside the params, or .grad touched"
    return stats.t


def bits(t):
    return t.detach().contiguous().view(torch.uint8).reshape(-1)


def same(a, b, sa, sb, what):
    """Optimisers a and b agree in every bit of the params and the state, and the stats too"""
    for x, y, name in ((a.pol, b.pol, "policy"), (a.crit, b.crit, "critic")):
        assert (x is None) == (y is None)
        assert x is None or torch.equal(bits(x.params), bits(y.params)), f"{what}: the {name}'s params"
    assert torch.equal(a.state, b.state), f"{what}: the optimiser state"
    assert torch.equal(bits(sa), bits(sb)), f"{what}: the stats"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", [(4, 16, 1), (6, 32, 2)])
def test_update_has_the_bits_of_the_loop(od, H, nh, f64):
    src = source(od, H, nh, f64)
    mbs = epochs()
    assert len(mbs) == 8 and sum(m.numel() for m in mbs) == 2 * N_SRC
    twin, opt = optimiser(src), optimiser(src, guarded=True)
    want = loop(twin, src, mbs)
    got = updated(opt, src, mbs)
    same(opt, twin, got, want, f"{od} {H} {nh}")
    head = opt.info()
    assert head["t"] == 8.0 and head["stopped"] == 0.0 and head["skipped_nonfinite"] == 0.0 and head["grad_norm"] > 0
    assert bool(torch.isfinite(got).all()) and got[:, 7].tolist() == [float(m.numel()) for m in mbs]
    assert not torch.equal(opt.pol.params, src["pol"].params) and not torch.equal(opt.crit.params, src["crit"].params)
    # a second call continues the same optimiser: the state is carried, and the workspace is reused
    want2, got2 = loop(twin, src, mbs[:3]), updated(opt, src, mbs[:3])
    same(opt, twin, got2, want2, "a second call")
    assert opt.info()["t"] == 11.0


@pytest.mark.parametrize("variant", ["no_old_values", "no_normalize", "policy_alone", "critic_alone", "empty_minibatch"])
def test_variants(variant):
    src = source(4, 32, 2, False)
    mbs = epochs(seed=12)
    nets = dict(pol=variant != "critic_alone", crit=variant != "policy_alone")
    kw = dict(old_values=variant not in ("no_old_values", "policy_alone"), normalize=variant != "no_normalize")
    if variant == "empty_minibatch":
        mbs = mbs[:2] + [torch.empty((0,), dtype=torch.int32, device=DEV)] + mbs[2:]
    twin, opt = optimiser(src, **nets), optimiser(src, guarded=True, **nets)
    want = loop(twin, src, mbs, **kw)
    got = updated(opt, src, mbs, **kw)
    same(opt, twin, got, want, variant)
    assert opt.info()["t"] == 8.0
    if variant == "empty_minibatch":
        assert got[2].tolist() == [0.0] * 8 and got[3, 7] > 0
    if variant == "no_normalize":  # the normalisation is not a no-op on these advantages (mean 0.3)
        other = optimiser(src, guarded=True)
        updated(other, src, mbs)
        assert not torch.equal(other.pol.params, opt.pol.params)
    if variant == "critic_alone":
        assert got[:, 1].tolist() == [0.0] * 8 and bool((got[:, 2] > 0).all())


def test_kl_stop_inside_the_call():
    src = dict(source(4, 32, 2, False))
    logits = torch.empty((N_SRC, 9), dtype=torch.float32, device=DEV)
    src["pol"].act(src["obs"], logits=logits)
    src["old_logp"] = padded(ppo.log_prob(logits, src["actions"].contiguous()).cpu().numpy())  # the ratio starts at 1 exactly
    mbs = epochs(seed=13)
    free = loop(optimiser(src), src, mbs)  # no gate: approx_kl of every minibatch as the params move
    kl = free[:, 4].cpu().numpy()
    assert kl[0] == 0.0 and bool((kl[1:] > 0).all()), "the first minibatch sees the rollout's own params"
    s = np.sort(kl)
    target = float(0.5 * (s[3] + s[4]))  # between the 4th and the 5th of 8: the stop falls inside the call
    at = int(np.argmax(kl > target))
    assert 1 <= at <= 4 and s[3] < target < s[4]
    twin, opt = optimiser(src, target_kl=target), optimiser(src, guarded=True, target_kl=target)
    want = loop(twin, src, mbs)
    got = updated(opt, src, mbs)
    same(opt, twin, got, want, "target_kl")
    head = opt.info()
    assert head["stopped"] == 1.0 and head["t"] == float(at), "the steps before the stop were applied, none after it"
    assert torch.equal(bits(got[:at + 1]), bits(free[:at + 1])), "up to the stop the stats are the ungated run's"
    # after the stop the launches still run and describe the unchanged params
    assert bool(torch.isfinite(got).all()) and got[at + 1:, 7].tolist() == [float(m.numel()) for m in mbs[at + 1:]]
    again = updated(opt, src, mbs[at:at + 1])
    assert torch.equal(bits(again[0]), bits(got[at])) and opt.info()["t"] == float(at), "stopped: a later call moves nothing"
    opt.resume()
    twin.resume()
    opt.target_kl = twin.target_kl = 1e3  # (the gate stays in the launch and never closes)
    same(opt, twin, updated(opt, src, mbs[:1]), loop(twin, src, mbs[:1]), "resumed")
    assert opt.info()["t"] == float(at + 1) and opt.info()["stopped"] == 0.0


def test_new_params_are_read_with_no_reregistration():
    E, N, K = 4, 8, 3
    vec = FlockVec(E, n_agents=[N], seed=37, device=DEV)
    src = source(vec.world.OD, 32, 2, False)
    opt = optimiser(src, guarded=True)
    pol = opt.pol
    vec.set_policy(pol)  # registered before the update, never again
    before = pol.act(src["obs"], logits=(lg0 := torch.empty((N_SRC, 9), dtype=torch.float32, device=DEV)))
    updated(opt, src, epochs(1, seed=14))
    fresh = plain_net(pol)  # another object with the updated values: what a re-registration would give
    lg1, lg2 = torch.empty_like(lg0), torch.empty_like(lg0)
    a1, a2 = pol.act(src["obs"], logits=lg1), fresh.act(src["obs"], logits=lg2)
    assert torch.equal(bits(lg1), bits(lg2)) and torch.equal(a1, a2) and not torch.equal(bits(lg1), bits(lg0))
    assert before.shape == a1.shape
    twin_vec = FlockVec(E, n_agents=[N], seed=37, device=DEV)
    twin_vec.set_policy(fresh)
    outs = []
    for v, net in ((vec, pol), (twin_vec, fresh)):
        acts = torch.empty((K + 1, E, N, 3), dtype=torch.uint8, device=DEV)
        net.act(v.obs, out=acts[0])
        lg = torch.empty((K, E, N, 9), dtype=torch.float32, device=DEV)
        traj = v.rollout_policy(acts, K, trajectory=True, logits=lg)
        outs.append((lg, acts, traj["obs"].clone()))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y)), "the rollout launch read the updated params"
    stale = plain_net(src["pol"])
    lg3 = torch.empty((E, N, 9), dtype=torch.float32, device=DEV)
    stale.act(twin_vec.obs, logits=lg3)
    pol.act(twin_vec.obs, logits=(lg4 := torch.empty_like(lg3)))
    assert not torch.equal(bits(lg3), bits(lg4))


def test_step_after_backward_has_the_bits_of_step_after_ppo_grads():
    src = source(4, 32, 2, False)
    mb = epochs(1, seed=15)[0].long()
    g = lambda k: src[k][mb].contiguous()
    a, b = optimiser(src), optimiser(src)
    for o in (a, b):
        o.pol.params.requires_grad_(True)
        o.crit.params.requires_grad_(True)
    sa = ppo.ppo_grads(a.pol, a.crit, g("obs"), g("actions"), g("old_logp"), g("adv"), g("ret"))
    a.step(sa)
    loss, sb = ppo.ppo_loss(b.pol.forward(g("obs")), b.crit.forward(g("obs")), g("actions"), g("old_logp"), g("adv"), g("ret"))
    loss.backward()
    assert torch.equal(bits(a.pol.params.grad), bits(b.pol.params.grad)) and torch.equal(bits(a.crit.params.grad), bits(b.crit.params.grad))
    b.step(sb)
    torch.cuda.synchronize()
    for x, y in ((a.pol, b.pol), (a.crit, b.crit)):
        assert torch.equal(bits(x.params), bits(y.params)) and not torch.equal(bits(x.params), bits(src["pol" if x is a.pol else "crit"].params))
    assert torch.equal(a.state, b.state) and a.info()["t"] == 1.0
    a.zero_grad()
    assert a.pol.params.grad is None and a.crit.params.grad is None
    with pytest.raises(ValueError, match="grad is None"):
        a.step()
