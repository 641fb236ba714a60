"""The MLP policy of include/macm.h (macm_policy_mlp) in numpy float32, written from the definition
and not from the kernel (tests/ only): the reference that macm_policy_flock and
macm_world_rollout_policy are compared with bit for bit.

    x[q]  = float32(obs[q])
    layer : acc = b[j]; acc = fma32(W[k][j], x[k], acc) for k ascending
    hidden: relu(v) = v if v > 0 else +0.0 (so -0 and NaN give +0); no activation on the 9 logits
    head h: z[c] = logits[3h + c] (+ noise[3h + c], one float32 add);
            best = 0, top = -inf; for c = 0, 1, 2: if z[c] > top: best, top = c, z[c]

fma32 is an exact float32 fused multiply-add without math.fma: the float64 product of two float32
values is exact (48 significant bits), the float64 sum of it and the addend is made round-to-odd with
the error term of TwoSum, and a round-to-odd float64 (53 bits >= 24 + 2) rounds to float32 as the exact
value would. IEEE 754 leaves the sign and payload of a generated NaN open and the definition does not fix
them either: a NaN here is some NaN, and comparisons with the device treat any two NaNs as equal
(same_bits)."""
import numpy as np

N_LOGITS = 9
F32, F64 = np.float32, np.float64


def same_bits(got, want):
    """Elementwise: the same float32 bit pattern, or both NaN."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def fma32(a, b, c):
    """round_to_nearest_even_float32(a * b + c), exactly, elementwise on float32 arrays."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(F64) * b.astype(F64)  # exact
        c64 = c.astype(F64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # TwoSum: p + c64 == s + err exactly
        s = np.array(s, F64, ndmin=1, copy=True)
        err = np.broadcast_to(err, s.shape)
        bits = s.view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        # the exact sum lies between s and its neighbour on err's side: round to odd takes that neighbour
        away = (err > 0) == (s > 0)  # the magnitude grows: sign-magnitude bits + 1
        bits[fix] += np.where(away, 1, -1)[fix]
        r = s.astype(F32)
    return r.reshape(np.broadcast(a, b, c).shape)


def relu(v):
    return np.where(v > 0, v, F32(0.0)).astype(F32)


def layer_shapes(in_dim, hidden, n_hidden):
    dims = [in_dim] + [hidden] * n_hidden + [N_LOGITS]
    return list(zip(dims[:-1], dims[1:]))


def n_params(in_dim, hidden, n_hidden):
    return sum(i * o + o for i, o in layer_shapes(in_dim, hidden, n_hidden))


def pack_params(weights, biases):
    """W[in][out] row-major then b, layer after layer: the flat float32 array of macm_policy_mlp.params."""
    return np.concatenate([np.concatenate([np.asarray(w, F32).reshape(-1), np.asarray(b, F32).reshape(-1)])
                           for w, b in zip(weights, biases)]).astype(F32)


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


def dense(W, b, x):
    """[rows, out]: the k-ordered fmaf chain of one layer over x [rows, in]."""
    acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[1])).astype(F32)
    for k in range(W.shape[0]):
        acc = fma32(W[k][None, :], x[:, k:k + 1], acc)
    return acc


def logits_of(params, in_dim, hidden, n_hidden, obs):
    """float32 [..., 9] for obs [..., in_dim] (float32 or float64 as stored)."""
    obs = np.asarray(obs)
    lead = obs.shape[:-1]
    x = obs.reshape(-1, in_dim).astype(F32)  # float64 rounds to nearest
    ws, bs = split_params(params, in_dim, hidden, n_hidden)
    for W, b in zip(ws[:-1], bs[:-1]):
        x = relu(dense(W, b, x))
    return dense(ws[-1], bs[-1], x).reshape(lead + (N_LOGITS,))


def actions_of(logits, noise=None):
    """uint8 [..., 3]: per head the lowest index of the largest z, by strict > from -inf."""
    z = np.asarray(logits, F32)
    if noise is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            z = (z + np.asarray(noise, F32)).astype(F32)
    z = z.reshape(z.shape[:-1] + (3, 3))
    best = np.zeros(z.shape[:-1], np.uint8)
    top = np.full(z.shape[:-1], -np.inf, F32)
    for c in range(3):
        with np.errstate(invalid="ignore"):
            m = z[..., c] > top
        best = np.where(m, np.uint8(c), best)
        top = np.where(m, z[..., c], top)
    return best.astype(np.uint8)


def policy(params, in_dim, hidden, n_hidden, obs, noise=None):
    """(actions uint8 [..., 3], logits float32 [..., 9])"""
    lg = logits_of(params, in_dim, hidden, n_hidden, obs)
    return actions_of(lg, noise), lg


# ---- the seeded weights and noise the tests share ---------------------------------------------------
# Flock's distances reach tens of metres, so unit-variance layers saturate the argmax: at scale 0.3 and
# with Gumbel noise, the reference closed loop of test_policy_ref.py takes every value of every head
# in more than 20% of the agent-steps, while the logits still decide a good part of them.
WEIGHT_SEED, WEIGHT_SCALE = 7, 0.3


def seeded_params(in_dim, hidden, n_hidden, seed=WEIGHT_SEED, scale=WEIGHT_SCALE):
    """Normal weights of standard deviation scale / sqrt(fan_in), biases of scale / 4."""
    rng = np.random.default_rng([seed, in_dim, hidden, n_hidden])
    ws, bs = [], []
    for i, o in layer_shapes(in_dim, hidden, n_hidden):
        ws.append((rng.standard_normal((i, o)) * (scale / np.sqrt(i))).astype(F32))
        bs.append((rng.standard_normal(o) * (scale / 4)).astype(F32))
    return pack_params(ws, bs)


def gumbel_noise(shape, seed):
    """float32 Gumbel(0, 1) noise: argmax(logits + noise) samples from softmax(logits)."""
    u = np.random.default_rng(seed).random(shape)
    return (-np.log(-np.log(np.clip(u, 1e-12, 1 - 1e-12)))).astype(F32)


def oracle_closed_loop(orc, params, in_dim, hidden, n_hidden, K, noise=None, reset=False):
    """The oracle's closed loop step -> policy -> step from its current state: the K + 1 action rows,
    the K logits rows and the steps' results. noise [K, E, N, 9] or None; reset: reset_envs on every
    step's done flags, the policy then acting on the new initial obs."""
    obs, _ = orc.observe()
    act, _ = policy(params, in_dim, hidden, n_hidden, obs)  # the first actions: the argmax on the initial obs
    arows, lrows, results = [act], [], []
    for k in range(K):
        r = orc.step(arows[-1])
        obs = r["obs"]
        if reset and r["done"].any():
            orc.reset_envs(r["done"])
            obs, _ = orc.observe()
        a, lg = policy(params, in_dim, hidden, n_hidden, obs, None if noise is None else noise[k])
        arows.append(a)
        lrows.append(lg)
        results.append(r)
    return np.stack(arows), np.stack(lrows), results
