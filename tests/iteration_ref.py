"""One PPO iteration as a textbook writes it (a helper, not a test): a gym-style collector and a torch learner
that know nothing about the row convention of the trajectory launches (include/macm.h), and the chain of the
suite's own references evaluated on the same tuples.

    collect(world, pol, crit, noise, T)   observe, decide, step: for every decision t the tuple
                                          (s_t, a_t, logits_t, v_t, r_t, done_t, v(s'_t)), s'_t before any reset
    gae(...), prepare(...), learn(...)    PPO from those tuples in torch on the CPU, float64 (or float32, to measure
                                          what the number format alone costs), with autograd, clip_grad_norm_ and
                                          torch.optim.Adam
    chain_step(...)                       minibatch_ref -> ppo_ref.loss -> grad_ref.grad: the definition of the
                                          device's first step on given rows, with grad_ref's bound

The collector is written against the one-shot calls of a world (``obs``, ``step``, ``reward``, ``done``,
``reset_envs``), a policy (``act``) and a critic (``value``); it is the only part that needs a device. Decision
t uses noise row t. A trajectory launch whose action row 0 is decision 0 therefore takes noise[1:]: its noise
row k belongs to decision k + 1.

The learner is deliberately plain: a functional MLP from the flat params (W [in][out] then b, layer after layer),
log_softmax over the three heads, the clipped surrogate, the clipped value loss where old values are used, the
entropy bonus, per-minibatch advantage normalisation with the unbiased std, one global-norm clip over both nets,
Adam. It rounds nothing to float32 on the way, where the library's definition rounds the log-probability and the
normalised advantage once each; test_iteration_ref.py bounds what those two roundings can change."""
import dataclasses

import numpy as np
import torch

import grad_ref as gr
import minibatch_ref as M
import ppo_ref as R

F32, F64 = np.float32, np.float64
STATS = R.STATS
FIELDS = ("obs", "actions", "logits", "values", "reward", "done", "next_value")


@dataclasses.dataclass
class Hyper:
    gamma: float = 0.99
    lam: float = 0.95
    clip: float = 0.2
    vf_coef: float = 0.5
    ent_coef: float = 0.01
    vf_clip: float = 0.2  # read only where old values are used
    adv_eps: float = 1e-8
    lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    max_grad_norm: float = 0.5

    def __post_init__(self):
        # The library takes gamma, lambda and the loss's coefficients as float32 (macm_gae's arguments,
        # macm_ppo_config's fields): clip=0.2 there is float32(0.2). These are inputs, not arithmetic, so the
        # textbook is handed the same numbers; Adam's hyperparameters are doubles on both sides.
        for f in ("gamma", "lam", "clip", "vf_coef", "ent_coef", "vf_clip"):
            setattr(self, f, float(F32(getattr(self, f))))


# ---- the collector ---------------------------------------------------------------------------------------
def collect(world, pol, crit, noise, T):
    """T decisions of every agent of `world`, a gym loop: observe, decide, step. noise: [T, E, N, 9] or None
    (argmax). Returns a dict of stacked device tensors, [T, ...] each (FIELDS): next_value is V of the obs the
    step produced, before the reset that follows an end."""
    rec = {f: [] for f in FIELDS}
    for t in range(T):
        s = world.obs.clone()                                   # observe
        logits = torch.empty(tuple(s.shape[:-1]) + (9,), dtype=torch.float32, device=s.device)
        a = pol.act(s, noise=None if noise is None else noise[t], logits=logits)  # decide
        v = crit.value(s)
        world.step(a)                                           # step
        r, done = world.reward.clone(), world.done.clone()
        nv = crit.value(world.obs)                              # s', whether or not the episode ended
        world.reset_envs(done.clone())                          # an ended env starts its next episode
        for f, x in zip(FIELDS, (s, a.clone(), logits, v, r, done, nv)):
            rec[f].append(x)
    return {f: torch.stack(x) for f, x in rec.items()}


def tuples_to_numpy(rec, lo=0, hi=None):
    """Decisions lo .. hi - 1 of collect()'s result as numpy arrays"""
    return {f: x[lo:hi].cpu().numpy() for f, x in rec.items()}


# ---- the learner -----------------------------------------------------------------------------------------
def gae(reward, values, next_value, done, gamma, lam, dtype=torch.float64):
    """(adv, ret) [T, E, N]: delta = r + gamma v(s') - v, A = delta + gamma lam (1 - done) A_next, ret = A + v,
    with done [T, E] and every end bootstrapping from the value of its own last observation"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    r, v, nv = t(reward), t(values), t(next_value)
    live = 1.0 - (torch.as_tensor(np.asarray(done)) != 0).to(dtype)[:, :, None]
    adv = torch.zeros_like(r)
    nxt = torch.zeros_like(r[0])
    for k in range(r.shape[0] - 1, -1, -1):
        delta = r[k] + gamma * nv[k] - v[k]
        nxt = delta + gamma * lam * live[k] * nxt
        adv[k] = nxt
    return adv, adv + v


def mlp(params, shapes, x):
    """The net's outputs [rows, out] from the flat params: relu on the hidden layers, none on the last"""
    at = 0
    for l, (i, o) in enumerate(shapes):
        W, b = params[at:at + i * o].view(i, o), params[at + i * o:at + i * o + o]
        at += i * o + o
        x = x @ W + b
        if l < len(shapes) - 1:
            x = torch.relu(x)
    assert at == params.numel()
    return x


def log_probs(logits, actions):
    """(logp [rows], entropy [rows]) of MultiDiscrete([3, 3, 3]) actions (long [rows, 3]) under logits [rows, 9]"""
    lp = torch.log_softmax(logits.view(-1, 3, 3), dim=-1)
    logp = lp.gather(-1, actions.view(-1, 3, 1)).squeeze(-1).sum(-1)
    return logp, -(lp.exp() * lp).sum((-1, -2))


def prepare(tup, hp, dtype=torch.float64):
    """The learner's rows from the collector's tuples (numpy, [T, E, N, ...]): flattened obs, actions, old_logp from
    the recorded logits, old_values, and adv and ret from gae, all in dtype"""
    adv, ret = gae(tup["reward"], tup["values"], tup["next_value"], tup["done"], hp.gamma, hp.lam, dtype)
    od = tup["obs"].shape[-1]
    actions = torch.as_tensor(tup["actions"]).long().view(-1, 3)
    old_logp, _ = log_probs(torch.as_tensor(tup["logits"]).to(dtype).view(-1, 9), actions)
    return dict(obs=torch.as_tensor(tup["obs"]).to(dtype).view(-1, od), actions=actions, old_logp=old_logp,
                old_values=torch.as_tensor(tup["values"]).to(dtype).view(-1), adv=adv.view(-1), ret=ret.view(-1))


def losses(pp, pc, pshapes, cshapes, rows, mb, hp, use_old_values, normalize=True):
    """(loss, stats [8] as tensors, the normalised advantages, their mean and std) of minibatch mb (long [n])"""
    obs, actions = rows["obs"][mb], rows["actions"][mb]
    adv, mean, std = rows["adv"][mb], None, None
    if normalize:
        mean, std = adv.mean(), adv.std()  # the unbiased std
        adv = (adv - mean) / (std + hp.adv_eps)
    logp, ent = log_probs(mlp(pp, pshapes, obs), actions)
    ratio = torch.exp(logp - rows["old_logp"][mb])
    policy_loss = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - hp.clip, 1 + hp.clip) * adv).mean()
    v, ret = mlp(pc, cshapes, obs).squeeze(-1), rows["ret"][mb]
    sq = (v - ret) ** 2
    if use_old_values:
        ov = rows["old_values"][mb]
        sq = torch.maximum(sq, (ov + torch.clamp(v - ov, -hp.vf_clip, hp.vf_clip) - ret) ** 2)
    value_loss = 0.5 * sq.mean()
    entropy = ent.mean()
    loss = policy_loss + hp.vf_coef * value_loss - hp.ent_coef * entropy
    with torch.no_grad():
        approx_kl = ((ratio - 1) - torch.log(ratio)).mean()
        clip_frac = ((ratio - 1).abs() > hp.clip).to(ratio.dtype).mean()
        stats = torch.stack([loss, policy_loss, value_loss, entropy, approx_kl, clip_frac, ratio.max(),
                             torch.tensor(float(len(mb)), dtype=ratio.dtype)])
    return loss, stats, adv, mean, std


def learn(rows, pol_params, crit_params, pshapes, cshapes, minibatches, hp, use_old_values=True,
          dtype=torch.float64, trace=None):
    """PPO over `minibatches` (index lists, one optimiser step each, in order). Returns (stats float64
    [n_mb, 8] in STATS order, the final policy params, the final critic params) as numpy arrays. trace: a list
    that receives per minibatch a dict of the gradients before the clip, the advantages' mean and std, the
    normalised advantages and the params after the step."""
    pp = torch.nn.Parameter(torch.as_tensor(np.asarray(pol_params)).to(dtype).clone())
    pc = torch.nn.Parameter(torch.as_tensor(np.asarray(crit_params)).to(dtype).clone())
    opt = torch.optim.Adam([pp, pc], lr=hp.lr, betas=hp.betas, eps=hp.eps, foreach=False)
    out = []
    for mb in minibatches:
        mb = torch.as_tensor(np.asarray(mb)).long()
        opt.zero_grad()
        loss, stats, advn, mean, std = losses(pp, pc, pshapes, cshapes, rows, mb, hp, use_old_values)
        loss.backward()
        grads = [pp.grad.detach().clone().numpy(), pc.grad.detach().clone().numpy()]
        if hp.max_grad_norm:
            torch.nn.utils.clip_grad_norm_([pp, pc], hp.max_grad_norm, foreach=False)
        opt.step()
        out.append(stats.to(torch.float64).numpy())
        if trace is not None:
            trace.append(dict(grads=grads, mean=float(mean), std=float(std), adv=advn.detach().numpy(),
                              params=[pp.detach().clone().numpy(), pc.detach().clone().numpy()]))
    return np.stack(out), pp.detach().numpy(), pc.detach().numpy()


# ---- the suite's references, chained ---------------------------------------------------------------------
def chain_step(rows, mb, pol_params, crit_params, pshape, vshape, hp, use_old_values=True):
    """The definition of the device's gradients of minibatch mb at float32 rows (numpy, flattened: obs, actions,
    logits and values of the nets as they stand, old_logp, adv, ret, old_values): minibatch_ref.moments and
    normalise, ppo_ref.loss, grad_ref.grad per net. pshape, vshape: (in_dim, hidden, n_hidden). Returns a dict:
    moments, adv (normalised, float32), loss (ppo_ref's dict), grad_policy and grad_value (float64) with their
    bounds tol_policy and tol_value (grad_ref.tol)."""
    mb = np.asarray(mb, np.int64)
    mom = M.moments(rows["adv"], mb, hp.adv_eps)
    advn = M.normalise(np.asarray(rows["adv"], F32).reshape(-1)[mb], mom["mean"], mom["rstd"])
    L = R.loss(rows["logits"][mb], rows["actions"][mb], rows["old_logp"][mb], advn, rows["values"][mb], rows["ret"][mb],
               rows["old_values"][mb] if use_old_values else None, clip=hp.clip, vf_coef=hp.vf_coef,
               ent_coef=hp.ent_coef, vf_clip=hp.vf_clip if use_old_values else None)
    gp, Gp = gr.grad(pol_params, *pshape, 9, rows["obs"][mb], L["dlogits"])
    gv, Gv = gr.grad(crit_params, *vshape, 1, rows["obs"][mb], L["dvalues"])
    n = len(mb)
    return dict(moments=mom, adv=advn, loss=L, grad_policy=gp, grad_value=gv, tol_policy=gr.tol(Gp, n, pshape[1]),
                tol_value=gr.tol(Gv, n, vshape[1]))
