"""The parameter gradients of include/macm.h (macm_policy_grad / macm_value_grad) in numpy, written from
the definition and not from the kernel (tests/ only).

    forward : policy_ref.dense / relu, the exact float32 forward; a_0 = float32(obs), a_l = relu(layer l)
    backward: d_L = dout; from the last layer to the first
        gW_l[k][j]    = sum_r a_{l-1}[r][k] d_l[r][j]
        gb_l[j]       = sum_r d_l[r][j]
        d_{l-1}[r][k] = sum_j W_l[k][j] d_l[r][j] if a_{l-1}[r][k] > 0 else 0         (l > 1 only)

The backward runs in float64 here. The device's is float32 with an association of its own, so the
comparison needs a bound, and the bound needs a magnitude: G is the same backward with every weight,
activation and dout replaced by its absolute value, i.e. per parameter the sum of the absolute values of
every product on every path into it. A float32 evaluation with at most n roundings on a path differs from
the exact value by at most about n 2^-24 G, whatever the association. The count:

    tol[p] = (rows + 2 hidden + 16) 2^-24 G[p]

at most `rows` roundings in the sum over rows, `hidden` and 9 in the two d chains, and slack. The kernel
(csrc/policy_grad.hip) stays inside that count: a weight gradient is one fmaf chain over the wave's rows
(at most `rows` steps, a tail lane adds exact zeros), a bias gradient a lane-local sum over the wave's tiles
and then 64 lanes (at most rows / 64 + 64 additions of nonzero terms: below rows + 16 for every rows, since
with one tile only min(rows, 64) terms are nonzero), and the partials are summed in float64 and rounded once.

With integer inputs (params in {-1, 0, 1}, obs in [-2, 2], dout in {-1, 0, 1}) every product and every
partial sum is an integer of magnitude at most G; while G.max() < 2^24 all of them are exact in float32, so
any association gives the same bits and the device must equal this reference bit for bit."""
import numpy as np

import policy_ref as pr
from policy_ref import F32, F64

N_OUT = {"policy": pr.N_LOGITS, "critic": 1}
SHAPES = [(od, h, nh) for od in (4, 6) for h in (16, 32) for nh in (1, 2)]  # 8 per net


def layer_shapes(in_dim, hidden, n_hidden, n_out):
    dims = [in_dim] + [hidden] * n_hidden + [n_out]
    return list(zip(dims[:-1], dims[1:]))


def n_params(in_dim, hidden, n_hidden, n_out):
    return sum(i * o + o for i, o in layer_shapes(in_dim, hidden, n_hidden, n_out))


def split_params(params, in_dim, hidden, n_hidden, n_out):
    params = np.asarray(params)
    assert params.shape == (n_params(in_dim, hidden, n_hidden, n_out),)
    ws, bs, at = [], [], 0
    for i, o in layer_shapes(in_dim, hidden, n_hidden, n_out):
        ws.append(params[at:at + i * o].reshape(i, o))
        at += i * o
        bs.append(params[at:at + o])
        at += o
    return ws, bs


def activations(params, in_dim, hidden, n_hidden, n_out, obs):
    """[a_0, a_1, (a_2)]: the float32 inputs of every layer, [rows, in] each, by the exact float32 forward.
    The forward is a function of the row alone, so it runs once per distinct row (integer inputs repeat)."""
    x = np.asarray(obs).reshape(-1, in_dim).astype(F32)  # float64 rounds to nearest
    ws, bs = split_params(np.asarray(params, F32), in_dim, hidden, n_hidden, n_out)
    uniq, inverse = np.unique(x, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    acts = [uniq]
    for W, b in zip(ws[:-1], bs[:-1]):
        acts.append(pr.relu(pr.dense(W, b, acts[-1])))
    return [a[inverse] for a in acts]


def backward(ws, acts, dout, dtype=F64):
    """The flat gradient in the layout of params, from the weights, the layers' inputs and dout [rows, n_out],
    everything converted to dtype first (float64: the reference; float32: a plain numpy backward)."""
    d = np.asarray(dout, dtype).reshape(acts[0].shape[0], -1)
    out = [None] * len(ws)
    for l in range(len(ws) - 1, -1, -1):
        a = np.asarray(acts[l], dtype)
        out[l] = np.concatenate([(a.T @ d).reshape(-1), d.sum(axis=0)])
        if l > 0:
            d = np.where(np.asarray(acts[l]) > 0, d @ np.asarray(ws[l], dtype).T, dtype(0))
    return np.concatenate(out).astype(dtype)


def grad(params, in_dim, hidden, n_hidden, n_out, obs, dout):
    """(g, G), float64 [n_params]: the reference gradient and its magnitude vector."""
    ws, _ = split_params(np.asarray(params, F32), in_dim, hidden, n_hidden, n_out)
    acts = activations(params, in_dim, hidden, n_hidden, n_out, obs)
    g = backward(ws, acts, dout)
    G = backward([np.abs(w) for w in ws], [np.abs(a) for a in acts], np.abs(np.asarray(dout, F64)))
    return g, G


def tol(G, rows, hidden):
    return (rows + 2 * hidden + 16) * 2.0 ** -24 * G


def live_fractions(acts):
    """Per hidden layer, the fraction of (row, unit) pairs with a positive activation."""
    return [float((a > 0).mean()) for a in acts[1:]]


# ---- the seeded inputs the tests share ---------------------------------------------------------------
def integer_inputs(net, in_dim, hidden, n_hidden, rows, seed=0):
    """(params, obs, dout) float32: params in {-1, 0, 1}, obs integers in [-2, 2], dout in {-1, 0, 1}."""
    n_out = N_OUT[net]
    rng = np.random.default_rng([seed, n_out, in_dim, hidden, n_hidden])  # the same net at every row count
    params = rng.integers(-1, 2, n_params(in_dim, hidden, n_hidden, n_out)).astype(F32)
    rng = np.random.default_rng([seed, n_out, in_dim, hidden, n_hidden, rows])
    obs = rng.integers(-2, 3, (rows, in_dim)).astype(F32)
    dout = rng.integers(-1, 2, (rows, n_out)).astype(F32)
    return params, obs, dout if n_out > 1 else dout[:, 0]


def float_inputs(net, in_dim, hidden, n_hidden, rows, seed=0):
    """(params, obs, dout) float32: params N(0, 0.3), obs 5 N(0, 1), dout N(0, 1)."""
    n_out = N_OUT[net]
    rng = np.random.default_rng([seed + 1000, n_out, in_dim, hidden, n_hidden])
    params = (0.3 * rng.standard_normal(n_params(in_dim, hidden, n_hidden, n_out))).astype(F32)
    rng = np.random.default_rng([seed + 1000, n_out, in_dim, hidden, n_hidden, rows])
    obs = (5.0 * rng.standard_normal((rows, in_dim))).astype(F32)
    dout = rng.standard_normal((rows, n_out)).astype(F32)
    return params, obs, dout if n_out > 1 else dout[:, 0]
