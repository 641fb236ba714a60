"""A whole PPO iteration, rollout_policy -> ppo.transitions -> gae -> ppo.update, against a textbook loop
(tests/iteration_ref.py) that knows nothing about the rows of a trajectory launch.

A twin world with the same seed runs the textbook collector (observe, decide, step, one noise row per decision);
the world under test runs one trajectory launch of K = 20 steps into guarded buffers. Half the envs are stepped
further than the others beforehand, so with time_limit = 0.25 (an episode ends at its 16th step) the ends fall at
rows 10 and 12 of the launch, inside it, and the launch restarts those envs itself.

1. ppo.transitions' rows are the textbook's tuples of decisions 1 .. K-1 bit for bit (decision 0 is the caller's,
   decision K is stepped by the next launch), gae on them is value_ref.gae on the tuples bit for bit, and the
   pairing that reads the staggered buffers row by row gives other advantages.
2. With old_logp from log_prob on the rows' own logits and actions the first minibatch of ppo.update reports
   ratio_max 1, approx_kl 0 and clip_frac 0 exactly; rows shifted by one against each other do not.
3. The device's first gradients (adv_moments -> ppo_grads(index=, adv_norm=)) lie within grad_ref.tol of the chain
   minibatch_ref -> ppo_ref.loss -> grad_ref.grad evaluated on the textbook's tuples: a derived bound.
4. Two epochs of four minibatches through ppo.update against the textbook learner (torch float64, autograd,
   clip_grad_norm_, torch.optim.Adam): `rows` exactly, clip_frac within 2 / rows (a count of threshold
   decisions), the other six stats within 8 times the largest gap, over the eight minibatches, between the
   same textbook code run in float32 and in float64, floored at 64 x 2^-24 of the stat's magnitude. The device
   is float32 storage with another association: the float32 textbook measures what that costs, and 8 leaves
   room for the association without hiding a shifted row, which misses by far more than 10 times that in
   value_loss or policy_loss (asserted). The final params are compared through these stats only: Adam's first
   steps are sign-like where a gradient is near zero, so a per-parameter tolerance would be arbitrary.

Measured on an MI355X ("A whole iteration"; every figure is printed before it is asserted): the
device's first gradients use at most 0.009 of grad_ref.tol; in test 4 the device is as far from the float64
textbook as the float32 textbook is and uses at most 0.18 of the allowed gap (approx_kl on the workgroup world),
clip_frac was equal in every minibatch, and the old pairing misses by 2,500 to 60,000 times the allowed gap.
With ppo.transitions replaced by the old pairing tests 1, 3 and 4 fail. Test 2 does not: the old pairing kept
obs, logits and actions of a decision together and misplaced values, reward, done and boot, which the ratio
does not see; test 2 guards obs or actions slipping against the logits."""
import functools

import numpy as np
import pytest
import torch

import iteration_ref as it
import policy_ref as pr
import value_ref as vr
from guard_bands import Guarded, GuardedOutputs
from test_gpu_rollout_autoreset import FKEYS, flock_twins
from test_gpu_rollout_policy import F64C, seeded_policy
from test_gpu_rollout_value import seeded_critic

pytestmark = pytest.mark.gpu

from gym_macm import ppo  # noqa: E402
from gym_macm.policy import gae  # noqa: E402

DEV = "cuda:0"
K, H, NH = 20, 32, 2
HP = it.Hyper(gamma=0.99, lam=0.95, lr=1e-3, max_grad_norm=0.5, vf_clip=0.2)
WORLDS = {
    "8x8polar": (8, 8, {}),
    "8x8f64cart": (8, 8, F64C),
    "16x64wave": (16, 64, {}),               # the full wave
    "2x96workgroup": (2, 96, {"start_spread": 12}),  # N > 64: the rollout is the launches of the loop
}
NAMES = list(WORLDS)


def bits(t):
    return t.detach().contiguous().view(torch.uint8).reshape(-1)


def clone_net(like):
    net = type(like)(like.in_dim, like.hidden, like.n_hidden, DEV)
    net.params.copy_(like.params.detach())
    return net


@functools.lru_cache(maxsize=None)
def collected(name):
    """The twin's textbook tuples and the launch's buffers of world `name`: computed once, read by every test"""
    E, N, kw = WORLDS[name]
    off, on = flock_twins(E, N, 19, time_limit=0.25, **kw)
    od = on.world.OD
    pol, crit = seeded_policy(od, H, NH), seeded_critic(od, H, NH)
    # 2 steps, new episodes in the odd envs, 3 more steps: the even envs are at their 5th step, the odd at their 3rd
    rng = np.random.default_rng([9400, E, N])
    pre = torch.from_numpy(rng.integers(0, 3, (5, E, N, 3)).astype(np.uint8)).to(DEV)
    odd = torch.tensor([e % 2 for e in range(E)], dtype=torch.uint8, device=DEV)
    for v in (off, on):
        for i in range(5):
            if i == 2:
                v.world.reset_envs(odd.clone())
            v.world.step(pre[i])
        assert not bool(v.world.done.any())
    assert torch.equal(bits(off.world.obs), bits(on.world.obs))
    noise = torch.from_numpy(pr.gumbel_noise((K + 1, E, N, 9), 5)).to(DEV)  # row t: decision t's
    rec = it.collect(off.world, pol, crit, noise, K)  # decisions 0 .. K-1, each stepped
    # the launch: action row 0 is decision 0, taken by the caller; its noise row k is decision k + 1's
    w = on.world
    on.set_policy(pol)
    on.set_critic(crit)
    acts, lg = Guarded((K + 1, E, N, 3), torch.uint8, DEV), Guarded((K, E, N, 9), torch.float32, DEV)
    vals, boot = Guarded((K + 1, E, N), torch.float32, DEV), Guarded((K, E, N), torch.float32, DEV)
    go = GuardedOutputs(w, FKEYS, n_steps=K)
    traj = {f: go[f] for f in FKEYS}
    pol.act(w.obs, noise=noise[0], out=acts.t[0])
    crit.value(w.obs, out=vals.t[0])
    torch.cuda.synchronize()
    got = on.rollout_policy(acts.t, K, noise=noise[1:], trajectory=True, traj=traj, logits=lg.t, values=vals.t,
                            boot=boot.t)
    torch.cuda.synchronize()
    go.check_bands(name)
    for what, g in (("actions", acts), ("logits", lg), ("values", vals), ("boot", boot)):
        assert g.bands_intact(), f"{name}: a store outside the {what} buffer"
    assert got is traj and on.status() == 0 and off.status() == 0
    t = ppo.transitions(traj, acts.t, lg.t, vals.t, boot.t)
    adv, ret = gae(t["reward"], t["values"], t["boot"], t["done"], HP.gamma, HP.lam)
    old_logp = ppo.log_prob(t["logits"], t["actions"])
    torch.cuda.synchronize()
    rows = (K - 1) * E * N
    g = torch.Generator().manual_seed(11)
    mbs = [mb for _ in range(2) for mb in ppo.minibatches(rows, 4, generator=g, block=64, device=DEV)]
    return dict(E=E, N=N, od=od, pol=pol, crit=crit, rec=rec, tup=it.tuples_to_numpy(rec, 1, K), traj=traj, acts=acts.t,
                lg=lg.t, vals=vals.t, boot=boot.t, t=t, adv=adv, ret=ret, old_logp=old_logp, rows=rows, mbs=mbs,
                keep=(off, on, acts, lg, vals, boot, go))


def old_pairing(c):
    """The rows as the staggered buffers read row by row, obs[k] beside reward[k] and values[k], cut to K - 1 rows"""
    adv, ret = gae(c["traj"]["reward"], c["vals"][:K], c["boot"], c["traj"]["done"], HP.gamma, HP.lam)
    actions = c["acts"][1:K]
    return dict(obs=c["traj"]["obs"][:K - 1], actions=actions, old_logp=ppo.log_prob(c["lg"][:K - 1], actions),
                adv=adv[:K - 1], ret=ret[:K - 1], old_values=c["vals"][:K - 1])


def aligned(c):
    t = c["t"]
    return dict(obs=t["obs"], actions=t["actions"], old_logp=c["old_logp"], adv=c["adv"], ret=c["ret"],
                old_values=t["values"])


def run_update(c, rows, mbs, use_old_values=True):
    """ppo.update from the seeded nets over rows (a dict as aligned()'s): the [len(mbs), 8] stats as numpy"""
    opt = ppo.Adam(clone_net(c["pol"]), clone_net(c["crit"]), lr=HP.lr, betas=HP.betas, eps=HP.eps,
                   max_grad_norm=HP.max_grad_norm)
    kw = dict(old_values=rows["old_values"], vf_clip=HP.vf_clip) if use_old_values else {}
    stats = ppo.update(opt, rows["obs"], rows["actions"], rows["old_logp"], rows["adv"], rows["ret"], minibatches=mbs,
                       adv_eps=HP.adv_eps, clip=HP.clip, vf_coef=HP.vf_coef, ent_coef=HP.ent_coef, **kw)
    torch.cuda.synchronize()
    assert opt.info()["t"] == float(len(mbs)) and opt.info()["skipped_nonfinite"] == 0.0
    return stats.cpu().numpy()


# ---- 1. the collector ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_transitions_are_the_textbook_tuples(name):
    c = collected(name)
    E, N, t, rec = c["E"], c["N"], c["t"], c["rec"]
    done = c["traj"]["done"].cpu().numpy() != 0
    assert done[1:K - 1].any(axis=0).all(), "every env ends at a row 1 <= k < K - 1 of the launch"
    ends = {int(k) for k in np.argwhere(done)[:, 0]}
    assert sorted(ends) == [10, 12], f"the even envs end at their 16th step, row 10, the odd at row 12: {sorted(ends)}"
    a = c["acts"].cpu().numpy()
    for h in range(3):
        assert sorted(np.unique(a[..., h]).tolist()) == [0, 1, 2], f"head {h} takes all three choices"
    # decision 0 is the caller's: the launch was given what the textbook did
    assert torch.equal(c["acts"][0], rec["actions"][0]) and torch.equal(bits(c["vals"][0]), bits(rec["values"][0]))
    # decisions 1 .. K-1
    for f, g in (("obs", "obs"), ("actions", "actions"), ("logits", "logits"), ("values", "values"),
                 ("reward", "reward"), ("done", "done"), ("boot", "next_value")):
        assert t[f].is_contiguous() and t[f].shape[0] == K - 1
        assert t[f].dtype == rec[g].dtype and tuple(t[f].shape) == tuple(rec[g][1:K].shape), f
        assert torch.equal(bits(t[f]), bits(rec[g][1:K])), f"{name}: {f} of the transitions is not the textbook's {g}"
    assert t["obs"].data_ptr() == c["traj"]["obs"].data_ptr() and t["values"].data_ptr() == c["vals"][1].data_ptr()
    # an end bootstraps from its own last observation, not from the next episode's first
    nxt, boot = bits(t["values"][1:]).view(K - 2, E, -1), bits(t["boot"][:-1]).view(K - 2, E, -1)
    same = (nxt == boot).all(dim=2).cpu().numpy()
    assert same[~done[1:K - 1]].all() and not same[done[1:K - 1]].any()
    # gae on the views is value_ref.gae on the tuples
    tup = c["tup"]
    want_adv, want_ret = vr.gae(tup["reward"], tup["values"], tup["next_value"], tup["done"], HP.gamma, HP.lam)
    assert pr.same_bits(c["adv"].cpu().numpy(), want_adv).all() and pr.same_bits(c["ret"].cpu().numpy(), want_ret).all()
    assert np.isfinite(want_adv).all() and len(np.unique(want_adv)) > c["rows"] // 2
    # the textbook's own float64 recursion agrees to float32's precision: the two GAEs are one function
    tb_adv, _ = it.gae(tup["reward"], tup["values"], tup["next_value"], tup["done"], HP.gamma, HP.lam)
    mag = np.abs(tup["reward"]).max() + 2 * np.abs(tup["values"]).max()
    assert np.abs(tb_adv.numpy() - want_adv).max() <= 4 * K * 2.0 ** -24 * mag / (1 - HP.gamma * HP.lam)
    # teeth: reading the staggered buffers row by row credits every reward to the following decision
    old = old_pairing(c)
    assert not torch.equal(bits(old["adv"]), bits(c["adv"]))
    assert float((old["adv"] != c["adv"]).float().mean()) > 0.5


# ---- 2. the first epoch's identities -------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_first_minibatch_sees_ratio_one(name):
    c = collected(name)
    rows, first = aligned(c), c["mbs"][:1]
    s = run_update(c, rows, first)[0]
    assert s[7] == first[0].numel() > 0
    assert s[6] == 1.0 and s[4] == 0.0 and s[5] == 0.0, f"ratio_max {s[6]!r} approx_kl {s[4]!r} clip_frac {s[5]!r}"
    # actions one row off the logits their old_logp came from, and obs one row off: neither reports them
    for what, shifted in (("actions", dict(rows, actions=c["acts"][:K - 1])),
                          ("obs", dict(rows, obs=c["traj"]["obs"][1:K]))):
        b = run_update(c, shifted, first)[0]
        assert b[6] > 1.0 and b[4] > 0.0, f"{what} shifted: ratio_max {b[6]!r} approx_kl {b[4]!r}"


# ---- 3. the first gradients against the chain of references --------------------------------------------
def numpy_rows(c):
    """The chain's float32 rows: the textbook's tuples, value_ref.gae on them, and the device's old_logp"""
    tup = c["tup"]
    adv, ret = vr.gae(tup["reward"], tup["values"], tup["next_value"], tup["done"], HP.gamma, HP.lam)
    return dict(obs=tup["obs"].reshape(-1, c["od"]), actions=tup["actions"].reshape(-1, 3), logits=tup["logits"].reshape(-1, 9),
                values=tup["values"].reshape(-1), old_values=tup["values"].reshape(-1),
                old_logp=c["old_logp"].cpu().numpy().reshape(-1), adv=adv.reshape(-1), ret=ret.reshape(-1))


@pytest.mark.parametrize("name", NAMES)
def test_first_gradients_within_the_derived_bound(name):
    c = collected(name)
    rows, mb = aligned(c), c["mbs"][0]
    pol, crit = clone_net(c["pol"]), clone_net(c["crit"])
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    norm = ppo.adv_moments(rows["adv"], mb, eps=HP.adv_eps)
    ppo.ppo_grads(pol, crit, rows["obs"], rows["actions"], rows["old_logp"], rows["adv"], rows["ret"],
                  old_values=rows["old_values"], clip=HP.clip, vf_coef=HP.vf_coef, ent_coef=HP.ent_coef,
                  vf_clip=HP.vf_clip, index=mb, adv_norm=norm)
    torch.cuda.synchronize()
    shape = (c["od"], H, NH)
    ch = it.chain_step(numpy_rows(c), mb.cpu().numpy(), c["pol"].params.cpu().numpy(), c["crit"].params.cpu().numpy(),
                       shape, shape, HP)
    assert not ch["loss"]["undecided"].any()
    for net, want, tol, what in ((pol, ch["grad_policy"], ch["tol_policy"], "policy"),
                                 (crit, ch["grad_value"], ch["tol_value"], "critic")):
        got = net.params.grad.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        share = float(np.max(err[tol > 0] / tol[tol > 0]))
        print(f"{name} {what}: the device's first gradient uses {share:.4f} of grad_ref.tol ({mb.numel()} rows)")
        assert np.isfinite(got).all() and np.abs(want).max() > 0 and (err <= tol).all(), what


# ---- 4. the whole update against the textbook learner --------------------------------------------------
@functools.lru_cache(maxsize=None)
def textbook(name, use_old_values):
    """(float64 stats, float32 stats) [8, 8] of the textbook learner on the textbook's tuples"""
    c = collected(name)
    mbs = [m.cpu().numpy() for m in c["mbs"]]
    pp, pc = c["pol"].params.cpu().numpy(), c["crit"].params.cpu().numpy()
    pshapes, cshapes = pr.layer_shapes(c["od"], H, NH), vr.layer_shapes(c["od"], H, NH)
    run = lambda dt: it.learn(it.prepare(c["tup"], HP, dt), pp, pc, pshapes, cshapes, mbs, HP, use_old_values, dt)[0]
    return run(torch.float64), run(torch.float32)


SIX = [0, 1, 2, 3, 4, 6]  # loss, policy_loss, value_loss, entropy, approx_kl, ratio_max


@pytest.mark.parametrize("use_old_values", [True, False], ids=["old_values", "no_old_values"])
@pytest.mark.parametrize("name", NAMES)
def test_update_follows_the_textbook_learner(name, use_old_values):
    c = collected(name)
    mbs = c["mbs"]
    assert len(mbs) == 8 and sum(m.numel() for m in mbs) == 2 * c["rows"]
    ref, ref32 = textbook(name, use_old_values)
    gap = np.abs(ref32 - ref).max(axis=0)        # what float32 alone costs the textbook, per stat
    allowed = np.maximum(8.0 * gap, 64 * 2.0 ** -24 * np.abs(ref).max(axis=0))
    got = run_update(c, aligned(c), mbs, use_old_values)
    err = np.abs(got - ref)
    used = err.max(axis=0)
    for i in SIX:
        print(f"{name} {'old_values' if use_old_values else 'no_old_values'} {it.STATS[i]}: float32 gap {gap[i]:.3e} "
              f"allowed {allowed[i]:.3e} device {used[i]:.3e} ({used[i] / allowed[i]:.3f} of it)")
    print(f"{name} clip_frac: device {got[:, 5].tolist()} textbook {ref[:, 5].tolist()}")
    assert np.isfinite(got).all() and got[:, 7].tolist() == ref[:, 7].tolist() == [float(m.numel()) for m in mbs]
    assert (np.abs(got[:, 5] - ref[:, 5]) <= 2.0 / ref[:, 7] + 1e-15).all(), "clip_frac: at most two rows decided otherwise"
    # (the textbook's first ratio is 1 to float32's precision only: its old_logp comes from the logits the float32
    # policy recorded, its new logp from a float64 forward pass)
    assert got[0, 6] == 1.0 and abs(ref[0, 6] - 1.0) <= allowed[6] and (ref[1:, 4] > 0).all(), "the params move after the first step"
    bad = [it.STATS[i] for i in SIX if not used[i] <= allowed[i]]
    assert not bad, f"{name}: {bad} outside 8 x the float32 gap: {used[SIX]} against {allowed[SIX]}"
    # the same update from the old pairing's rows misses by more than 10 times that
    miss = np.abs(run_update(c, old_pairing(c), mbs, use_old_values) - ref).max(axis=0)
    print(f"{name} old pairing: policy_loss misses by {miss[1] / allowed[1]:.1f} x allowed, value_loss by {miss[2] / allowed[2]:.1f} x")
    assert miss[1] > 10 * allowed[1] or miss[2] > 10 * allowed[2]
