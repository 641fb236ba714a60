"""The critic of include/macm.h (macm_value_mlp) and macm_gae in numpy float32, written from the
definitions and not from the kernels (tests/ only): the reference that macm_value_flock,
macm_world_rollout_policy_value and macm_gae are compared with bit for bit.

The critic is the policy's arithmetic (policy_ref: fma32, dense, relu) with one output and no head:

    x[q]  = float32(obs[q])
    layer : acc = b[j]; acc = fma32(W[k][j], x[k], acc) for k ascending
    hidden: relu(v) = v if v > 0 else +0.0; no activation on the last layer, whose one output is V

GAE, all float32, gl = gamma * lambda (one multiply), carry = +0.0, for k from K - 1 down to 0:

    delta  = fma32(gamma, boot[k], reward[k]) - values[k]
    adv[k] = delta if done[k, e] else fma32(gl, carry, delta)
    ret[k] = adv[k] + values[k]
    carry  = adv[k]

A NaN is some NaN (policy_ref.same_bits)."""
import numpy as np

import policy_ref as pr
from policy_ref import F32

WEIGHT_SEED = 13  # the critic's seeded weights: not the actor's


def layer_shapes(in_dim, hidden, n_hidden):
    dims = [in_dim] + [hidden] * n_hidden + [1]
    return list(zip(dims[:-1], dims[1:]))


def n_params(in_dim, hidden, n_hidden):
    return sum(i * o + o for i, o in layer_shapes(in_dim, hidden, n_hidden))


def split_params(params, in_dim, hidden, n_hidden):
    params = np.asarray(params, F32)
    assert params.shape == (n_params(in_dim, hidden, n_hidden),)
    ws, bs, at = [], [], 0
    for i, o in layer_shapes(in_dim, hidden, n_hidden):
        ws.append(params[at:at + i * o].reshape(i, o))
        at += i * o
        bs.append(params[at:at + o])
        at += o
    return ws, bs


def value_of(params, in_dim, hidden, n_hidden, obs):
    """float32 [...] for obs [..., in_dim] (float32 or float64 as stored)."""
    obs = np.asarray(obs)
    lead = obs.shape[:-1]
    x = obs.reshape(-1, in_dim).astype(F32)  # float64 rounds to nearest
    ws, bs = split_params(params, in_dim, hidden, n_hidden)
    for W, b in zip(ws[:-1], bs[:-1]):
        x = pr.relu(pr.dense(W, b, x))
    return pr.dense(ws[-1], bs[-1], x)[:, 0].reshape(lead)


def seeded_params(in_dim, hidden, n_hidden, seed=WEIGHT_SEED, scale=pr.WEIGHT_SCALE):
    """As policy_ref.seeded_params, for the critic's shapes and from another seed."""
    rng = np.random.default_rng([seed, in_dim, hidden, n_hidden])
    ws, bs = [], []
    for i, o in layer_shapes(in_dim, hidden, n_hidden):
        ws.append((rng.standard_normal((i, o)) * (scale / np.sqrt(i))).astype(F32))
        bs.append((rng.standard_normal(o) * (scale / 4)).astype(F32))
    return pr.pack_params(ws, bs)


def gae(reward, values, boot, done, gamma, lam):
    """(adv, ret) float32 [K, E, N] from reward, values, boot [K, E, N] and done [K, E] (nonzero: done)."""
    reward, values, boot = (np.asarray(v, F32) for v in (reward, values, boot))
    done = np.asarray(done) != 0
    K = reward.shape[0]
    gamma, lam = F32(gamma), F32(lam)
    gl = F32(gamma * lam)
    adv, ret = np.empty_like(reward), np.empty_like(reward)
    carry = np.zeros(reward.shape[1:], F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(K - 1, -1, -1):
            delta = (pr.fma32(gamma, boot[k], reward[k]) - values[k]).astype(F32)
            a = np.where(done[k][:, None], delta, pr.fma32(gl, carry, delta)).astype(F32)
            adv[k] = a
            ret[k] = (a + values[k]).astype(F32)
            carry = a
    return adv, ret

