"""The TDM set policy of include/macm.h (macm_tdm_policy) in numpy float32, written from the definition
and not from the kernel (tests/ only): the reference that macm_policy_tdm and macm_tdm_rollout_policy
are compared with bit for bit. fma32, relu and same_bits are tests/policy_ref.py's.

    for every slot k with m[k] != 0: e_k[j] = relu(b1[j] + sum_q W1[q][j] o[k][q]), q = 0..3 ascending
    g[j] = +0; g[j] = e_k[j] if e_k[j] > g[j] else g[j], over the live slots
    u = (g[0..H-1], float32(health)); t[j] = relu(b2[j] + sum_k W2[k][j] u[k]), k = 0..H ascending
    z[c] = b3[c] + sum_k W3[k][c] t[k]; heads 0..2 at z[3h + c], head 3 at z[9], z[10]
    action[h]: best = 0, top = -inf; for c ascending: if z[c] (+ noise[c]) > top: best, top = c, z[c]
"""
import numpy as np

from policy_ref import F32, dense, fma32, relu, same_bits  # noqa: F401  (re-exported for the tests)

N_LOGITS = 11
HEADS = ((0, 3), (3, 3), (6, 3), (9, 2))  # (first logit, choices) of MultiDiscrete([3, 3, 3, 2])


def layer_shapes(hidden):
    return [(4, hidden), (hidden + 1, hidden), (hidden, N_LOGITS)]


def n_params(hidden):
    return sum(i * o + o for i, o in layer_shapes(hidden))


def pack_params(weights, biases):
    return np.concatenate([np.concatenate([np.asarray(w, F32).reshape(-1), np.asarray(b, F32).reshape(-1)])
                           for w, b in zip(weights, biases)]).astype(F32)


def split_params(params, hidden):
    params = np.asarray(params, F32)
    assert params.shape == (n_params(hidden),)
    ws, bs, at = [], [], 0
    for i, o in layer_shapes(hidden):
        ws.append(params[at:at + i * o].reshape(i, o))
        at += i * o
        bs.append(params[at:at + o])
        at += o
    return ws, bs


def pooled(params, hidden, obs, mask):
    """float32 [rows, H]: the pool over the live slots of obs [rows, S, 4] under mask [rows, S]."""
    (W1, _, _), (b1, _, _) = split_params(params, hidden)
    rows, S = mask.shape
    g = np.zeros((rows, hidden), F32)
    for k in range(S):  # slot by slot, as the definition; the masked slots are never looked at
        live = mask[:, k] != 0
        if not live.any():
            continue
        e = relu(dense(W1, b1, obs[live, k, :].astype(F32)))
        cur = g[live]
        g[live] = np.where(e > cur, e, cur)
    return g


def logits_of(params, hidden, obs, mask, health):
    """float32 [..., N, 11] for obs [..., N, N-1, 4] (float32 or float64 as stored), mask [..., N, N-1] and
    health [..., N] (float64)."""
    obs, mask, health = np.asarray(obs), np.asarray(mask), np.asarray(health)
    lead = health.shape
    S = obs.shape[-2]
    o = obs.reshape(-1, S, 4)
    m = mask.reshape(-1, S)
    h = health.reshape(-1).astype(np.float64).astype(F32)  # the double rounds to nearest
    ws, bs = split_params(params, hidden)
    g = pooled(params, hidden, o, m)
    u = np.concatenate([g, h[:, None]], axis=1).astype(F32)  # the health is input k = H
    t = relu(dense(ws[1], bs[1], u))
    return dense(ws[2], bs[2], t).reshape(lead + (N_LOGITS,))


def actions_of(logits, noise=None):
    """uint8 [..., 4]: per head the lowest index of the largest z, by strict > from -inf."""
    z = np.asarray(logits, F32)
    if noise is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            z = (z + np.asarray(noise, F32)).astype(F32)
    out = np.zeros(z.shape[:-1] + (4,), np.uint8)
    for h, (at, n) in enumerate(HEADS):
        best = np.zeros(z.shape[:-1], np.uint8)
        top = np.full(z.shape[:-1], -np.inf, F32)
        for c in range(n):
            with np.errstate(invalid="ignore"):
                m = z[..., at + c] > top
            best = np.where(m, np.uint8(c), best)
            top = np.where(m, z[..., at + c], top)
        out[..., h] = best
    return out


def policy(params, hidden, obs, mask, health, noise=None):
    """(actions uint8 [..., N, 4], logits float32 [..., N, 11])"""
    lg = logits_of(params, hidden, obs, mask, health)
    return actions_of(lg, noise), lg


# ---- the seeded weights and noise the tests share ---------------------------------------------------
# A TDM slot is (r, t, health, ally): distances of up to tens of metres, so the encoder's scale is kept
# below unit variance as policy_ref.py's is; with Gumbel noise every head takes every value.
WEIGHT_SEED, WEIGHT_SCALE = 11, 0.5


def seeded_params(hidden, seed=WEIGHT_SEED, scale=WEIGHT_SCALE):
    """Normal weights of standard deviation scale / sqrt(fan_in), biases of scale / 4."""
    rng = np.random.default_rng([seed, hidden])
    ws, bs = [], []
    for i, o in layer_shapes(hidden):
        ws.append((rng.standard_normal((i, o)) * (scale / np.sqrt(i))).astype(F32))
        bs.append((rng.standard_normal(o) * (scale / 4)).astype(F32))
    return pack_params(ws, bs)


def gumbel_noise(shape, seed):
    """float32 Gumbel(0, 1) noise: argmax(logits + noise) samples from softmax(logits)."""
    u = np.random.default_rng(seed).random(shape)
    return (-np.log(-np.log(np.clip(u, 1e-12, 1 - 1e-12)))).astype(F32)


# The autoreset case with combat ends that tests/test_gpu_tdm_rollout_policy.py runs on the device: an 8 x 8
# world, teams [4, 4], the policy (H = 32, Gumbel noise of seed 5) on team 0 against bots.combat on team 1.
# tests/test_tdm_policy_ref.py checks on the CPU, with the oracle and this reference, that within K steps
# episodes end by combat, at more than one step, and that a reset env's terminal health differs from
# init_health among the policy's agents: a policy that read the step's health output would decide otherwise.
# (Four hits a second apart end an agent at the default damage and cooldown: the first episodes end at step
# 183, two envs, and at step 244, six more.)
COMBAT_CASE = dict(teams=[4, 4], E=16, seed=31, K=250, H=32, noise_seed=5,
                   cfg=dict(world_width=8.0, world_height=8.0))


def oracle_closed_loop(orc, bot, params, hidden, agents, K, noise, init_health):
    """The oracle's per-step loop step -> reset_envs(done) -> bot (everyone) -> policy (the agents whose entry
    in `agents` [N] is set, over the bot's actions): the K + 1 action rows and the steps' results, the
    terminal health among them. The policy of a reset env reads init_health."""
    agents = np.asarray(agents, bool)
    obs, mask = orc.observe()
    health = np.full(mask.shape[:2], init_health, np.float64)
    act = bot(obs, mask)
    act[:, agents] = policy(params, hidden, obs, mask, health)[0][:, agents]  # the first actions: the argmax
    arows, results = [act.copy()], []
    for k in range(K):
        r = orc.step(arows[-1])
        obs, mask, health = r["obs"], r["mask"], r["health"].copy()
        if r["done"].any():
            orc.reset_envs(r["done"])
            obs, mask = orc.observe()
            health[r["done"].astype(bool)] = init_health
        act = bot(obs, mask)
        act[:, agents] = policy(params, hidden, obs, mask, health, noise[k])[0][:, agents]
        arows.append(act.copy())
        results.append(r)
    return np.stack(arows), results


def logits_f64(params, hidden, obs, mask, health):
    """The same function in float64 numpy, plain sums (what torch_logits is held to in float64)."""
    ws, bs = split_params(params, hidden)
    W1, W2, W3 = (w.astype(np.float64) for w in ws)
    b1, b2, b3 = (b.astype(np.float64) for b in bs)
    o = np.asarray(obs, np.float64)
    live = np.asarray(mask) != 0
    e = np.maximum(np.where(live[..., None], o, 0.0) @ W1 + b1, 0.0)
    e = np.where(live[..., None], e, 0.0)
    g = e.max(axis=-2) if e.shape[-2] else np.zeros(e.shape[:-2] + e.shape[-1:])
    h = np.asarray(health, np.float64).astype(F32).astype(np.float64)
    u = np.concatenate([g, h[..., None]], axis=-1)
    return np.maximum(u @ W2 + b2, 0.0) @ W3 + b3
