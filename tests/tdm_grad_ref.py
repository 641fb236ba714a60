"""The parameter gradients of the TDM set policy (include/macm.h, macm_tdm_policy_grad) in numpy, written
from the definition and not from the kernel (tests/ only).

    forward : tdm_policy_ref's exact float32 forward: o = float32(obs), e_k over the live slots, the pool g,
              u = (g, float32(health)), t = relu(layer 2); the logits themselves are not needed
    backward: d3 = dlogits of the row, then
        gW3[k][c] = sum_r t[r][k] d3[r][c]                gb3[c] = sum_r d3[r][c]
        d2[r][j]  = sum_c W3[j][c] d3[r][c] if t[r][j] > 0 else 0
        gW2[k][j] = sum_r u[r][k] d2[r][j], k = 0..H      gb2[j] = sum_r d2[r][j]      (row H: the health)
        dg[r][j]  = sum_i W2[j][i] d2[r][i] if g[r][j] > 0 else 0
        winner k*(r, j): the lowest live slot k with e_k[j] == g[j], only when g[j] > 0
        gW1[q][j] = sum_r o[r][k*][q] dg[r][j]            gb1[j] = sum_r dg[r][j]      over (r, j) with a winner
    A row whose agents[row % N] is 0 takes no part: nothing of it is read.

The backward runs in float64 here. G is the same backward with every weight, activation, slot value and
dlogit replaced by its absolute value: per parameter the sum of the absolute values of every product on every
path into it. A float32 evaluation with at most n roundings on a path differs from the exact value by at most
about n 2^-24 G, whatever the association:

    tol[p] = (rows + 2 hidden + 16) 2^-24 G[p]

The count for csrc/tdm_policy_grad.hip: the d2 chain rounds 11 times and the dg chain `hidden` times; a layer-1
term o[k*][q] dg[j] rounds once; a weight gradient of layers 2 and 3 is one fmaf chain over the wave's rows, a
layer-1 gradient one chain of additions over the wave's rows and gb3 a lane-local sum over the wave's tiles and
then 64 lanes: at most `rows` roundings each (a tail lane, a skipped row and a unit without a winner add exact
zeros). The partials are summed in float64 and rounded once. The largest path, into W1, has at most
rows + hidden + 11 + 2 roundings: inside rows + 2 hidden + 16 for both hidden sizes.

With integer inputs every product and partial sum is an integer of magnitude at most G; while G.max() < 2^24
all of them are exact in float32, any association gives the same bits, and the device must equal this reference
bit for bit, ties included.

The keyword arguments of `grad` after `agents` state four wrong definitions (the highest tied slot wins, every
tied slot takes the gradient, masked slots take part, the health row is dropped): tests/test_tdm_grad_ref.py
checks that its constructed rows tell each of them from the definition."""
import numpy as np

import tdm_policy_ref as tp
from tdm_policy_ref import F32, N_LOGITS, dense, n_params, relu, split_params  # noqa: F401

F64 = np.float64


def forward(params, hidden, obs, mask, health, agents=None, use_mask=True):
    """The stored activations of every row, float32: dict(o [rows, S, 4], live [rows, S], keep [rows],
    e [rows, S, H] (zeros where not live), g [rows, H], u [rows, H + 1], t [rows, H]). Masked slots and the
    rows of skipped agents are never read: what they hold is replaced by zeros before anything looks at it."""
    obs, mask = np.asarray(obs), np.asarray(mask)
    S = mask.shape[-1]
    m = mask.reshape(-1, S)
    rows = m.shape[0]
    N = S + 1
    keep = np.ones(rows, bool) if agents is None else np.asarray(agents)[np.arange(rows) % N] != 0
    live = (m != 0) if use_mask else np.ones_like(m, bool)
    live = live & keep[:, None]
    o = np.zeros((rows, S, 4), F32)
    o[live] = obs.reshape(rows, S, 4)[live].astype(F32)  # a float64 slot rounds to nearest
    h = np.zeros(rows, F32)
    h[keep] = np.asarray(health, F64).reshape(-1)[keep].astype(F32)
    # the forward is a function of the row alone, so it runs once per distinct row (integer inputs repeat)
    key = np.concatenate([o.reshape(rows, -1), live.astype(F32), h[:, None]], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    uo, ulive, uh = uniq[:, :S * 4].reshape(-1, S, 4), uniq[:, S * 4:S * 5] != 0, uniq[:, -1]
    ws, bs = split_params(params, hidden)
    e = np.zeros((uniq.shape[0], S, hidden), F32)
    if ulive.any():
        e[ulive] = relu(dense(ws[0], bs[0], uo[ulive]))
    g = tp.pooled(params, hidden, uo, ulive.astype(np.uint8))  # the pool as tdm_policy_ref states it
    u = np.concatenate([g, uh[:, None]], axis=1).astype(F32)
    t = relu(dense(ws[1], bs[1], u))
    e, g, u, t = e[inverse], g[inverse], u[inverse], t[inverse]
    return dict(o=o, live=live, keep=keep, e=e, g=g, u=u, t=t)


def forward_f64(params, hidden, obs, mask, health):
    """The same dict with float64 plain-sum activations of the float32 inputs (what torch_logits computes on a
    float64 copy of the params): for the comparison with torch.autograd, not for the device."""
    obs, mask = np.asarray(obs), np.asarray(mask)
    S = mask.shape[-1]
    live = mask.reshape(-1, S) != 0
    rows = live.shape[0]
    o = np.where(live[:, :, None], obs.reshape(rows, S, 4).astype(F32).astype(F64), 0.0)
    ws, bs = split_params(params, hidden)
    e = np.where(live[:, :, None], np.maximum(o @ ws[0].astype(F64) + bs[0].astype(F64), 0.0), 0.0)
    g = e.max(axis=1) if S else np.zeros((rows, hidden))
    h = np.asarray(health, F64).reshape(-1).astype(F32).astype(F64)
    u = np.concatenate([g, h[:, None]], axis=1)
    t = np.maximum(u @ ws[1].astype(F64) + bs[1].astype(F64), 0.0)
    return dict(o=o, live=live, keep=np.ones(rows, bool), e=e, g=g, u=u, t=t)


def receivers(fwd, tie="lowest"):
    """bool [rows, S, H]: the slots that take unit j's gradient. The definition: the lowest live slot whose
    e equals a positive g. tie = "highest" / "all": the wrong rules the tests must tell from it."""
    tied = fwd["live"][:, :, None] & (fwd["e"] == fwd["g"][:, None, :]) & (fwd["g"] > 0)[:, None, :]
    if tie == "all":
        return tied
    first = np.cumsum(tied, axis=1) == 1 if tie == "lowest" else np.cumsum(tied[:, ::-1], axis=1)[:, ::-1] == 1
    return tied & first


def tied_units(fwd):
    """How many (row, unit) pairs have two or more live slots of different content at the pool's value."""
    tied = fwd["live"][:, :, None] & (fwd["e"] == fwd["g"][:, None, :]) & (fwd["g"] > 0)[:, None, :]
    lo, hi = receivers(fwd, "lowest"), receivers(fwd, "highest")
    both = tied.sum(axis=1) >= 2
    # the lowest and the highest tied slot's contents, per (row, unit)
    o_lo = np.einsum("rkj,rkq->rjq", lo.astype(F64), fwd["o"].astype(F64))
    o_hi = np.einsum("rkj,rkq->rjq", hi.astype(F64), fwd["o"].astype(F64))
    return int((both & (o_lo != o_hi).any(axis=2)).sum())


def backward(ws, fwd, dlogits, recv, absolute=False, health_row=True):
    """The flat float64 gradient in the layout of params. absolute: the magnitude vector's backward."""
    a = np.abs if absolute else (lambda v: v)
    W1, W2, W3 = (a(w.astype(F64)) for w in ws)
    H = W1.shape[1]
    keep = fwd["keep"]
    d3 = np.zeros((keep.shape[0], N_LOGITS), F64)
    d3[keep] = a(np.asarray(dlogits, F32).reshape(-1, N_LOGITS)[keep].astype(F64))
    t, u, g, o = (a(fwd[k].astype(F64)) for k in ("t", "u", "g", "o"))
    gW3, gb3 = t.T @ d3, d3.sum(axis=0)
    d2 = np.where(fwd["t"] > 0, d3 @ W3.T, 0.0)
    gW2, gb2 = u.T @ d2, d2.sum(axis=0)
    if not health_row:
        gW2[H] = 0.0
    dg = np.where(fwd["g"] > 0, d2 @ W2[:H].T, 0.0)
    r = recv.astype(F64)
    ow = np.einsum("rkq,rkj->rjq", o, r)  # per (row, unit) the receiving slot's content (zeros: no receiver)
    gW1 = np.einsum("rjq,rj->qj", ow, dg)
    gb1 = (r.sum(axis=1) * dg).sum(axis=0)
    return np.concatenate([gW1.reshape(-1), gb1, gW2.reshape(-1), gb2, gW3.reshape(-1), gb3])


def grad(params, hidden, obs, mask, health, dlogits, agents=None, tie="lowest", use_mask=True, health_row=True):
    """(g, G), float64 [n_params]: the reference gradient and its magnitude vector."""
    ws, _ = split_params(params, hidden)
    fwd = forward(params, hidden, obs, mask, health, agents, use_mask)
    recv = receivers(fwd, tie)
    return (backward(ws, fwd, dlogits, recv, False, health_row),
            backward(ws, fwd, dlogits, recv, True, health_row))


def tol(G, rows, hidden):
    return (rows + 2 * hidden + 16) * 2.0 ** -24 * G


def layer_slices(hidden):
    """name -> slice of the flat gradient: W1, b1, W2, b2, W3, b3."""
    out, at = {}, 0
    for l, (i, o) in enumerate(tp.layer_shapes(hidden), 1):
        out[f"W{l}"] = slice(at, at + i * o)
        out[f"b{l}"] = slice(at + i * o, at + i * o + o)
        at += i * o + o
    return out


# ---- the seeded inputs the tests share ---------------------------------------------------------------
def seeded_mask(rng, envs, n_agents):
    """uint8 [E, N, N-1]: about one agent in five is dead (its own slots and its slot in every other row are
    0); agent 0 of env 0 sees nobody (the empty set) whatever the draw."""
    alive = rng.random((envs, n_agents)) < 0.8
    other = np.array([[j for j in range(n_agents) if j != i] for i in range(n_agents)])  # [N, N-1]
    mask = (alive[:, :, None] & alive[:, other]).astype(np.uint8)
    mask[0, 0, :] = 0
    return mask


INT_DENSITY_ROWS = 1500  # integer inputs: about this many rows carry a nonzero dlogits row, however many rows


def integer_inputs(hidden, n_agents, envs, seed=0):
    """dict(params, obs float32 [E, N, N-1, 4], mask, health float64 [E, N], dlogits float32 [E, N, 11]):
    params in {-1, 0, 1}, slot values integers in [-2, 2], health in {0, 1, 2}, dlogits in {-1, 0, 1} on about
    INT_DENSITY_ROWS rows (all of them below that) and zeros elsewhere, so that G stays below 2^24 at every
    row count (checked by the tests that rely on it). Few distinct slot values: ties abound."""
    rng = np.random.default_rng([seed, hidden])  # the same net at every shape
    params = rng.integers(-1, 2, n_params(hidden)).astype(F32)
    rng = np.random.default_rng([seed, hidden, n_agents, envs])
    S, rows = n_agents - 1, envs * n_agents
    obs = rng.integers(-2, 3, (envs, n_agents, S, 4)).astype(F32)
    health = rng.integers(0, 3, (envs, n_agents)).astype(F64)
    dl = rng.integers(-1, 2, (envs, n_agents, N_LOGITS)).astype(F32)
    dl *= (rng.random((envs, n_agents, 1)) < min(1.0, INT_DENSITY_ROWS / rows)).astype(F32)
    return dict(params=params, obs=obs, mask=seeded_mask(rng, envs, n_agents), health=health, dlogits=dl)


def float_inputs(hidden, n_agents, envs, seed=0):
    """As integer_inputs with tdm_policy_ref's seeded normal weights, obs float64 3 N(0, 1) (not float32
    values: a float64 call rounds them, a float32 call takes obs.astype(float32)), health in [0, 1) and dlogits
    N(0, 1)."""
    params = tp.seeded_params(hidden, seed=tp.WEIGHT_SEED + seed)
    rng = np.random.default_rng([seed + 1000, hidden, n_agents, envs])
    S = n_agents - 1
    obs = 3.0 * rng.standard_normal((envs, n_agents, S, 4))
    health = rng.random((envs, n_agents))
    dl = rng.standard_normal((envs, n_agents, N_LOGITS)).astype(F32)
    return dict(params=params, obs=obs, mask=seeded_mask(rng, envs, n_agents), health=health, dlogits=dl)


# ---- constructed rows: one property each, for the reference's own tests and for the device -------------
def selector_params(hidden):
    """A net by hand: unit 0 of the encoder reads coordinate 0 alone (e_k[0] = relu(o[k][0])), unit 1 is
    relu(o[k][1] - 1), the others are off (bias -1, no weights). Layer 2 passes g[0] and g[1] on to t[0], t[1]
    (W2[j][j] = 1) and adds the health to t[2] (bias 0.5); layer 3 sums t[0..2] into every logit."""
    H = hidden
    W1, b1 = np.zeros((4, H), F32), np.full(H, -1.0, F32)
    W1[0, 0], b1[0] = 1.0, 0.0
    W1[1, 1], b1[1] = 1.0, -1.0
    W2, b2 = np.zeros((H + 1, H), F32), np.zeros(H, F32)
    W2[0, 0] = W2[1, 1] = 1.0
    W2[H, 2], b2[2] = 1.0, 0.5
    W3, b3 = np.zeros((H, N_LOGITS), F32), np.zeros(N_LOGITS, F32)
    W3[0:3, :] = 1.0
    return tp.pack_params([W1, W2, W3], [b1, b2, b3])


def constructed_case(name, hidden):
    """dict(params, obs [E, N, N-1, 4] float32, mask, health, dlogits, agents or None) of one env of N = 3
    agents (two slots per row) on selector_params; dlogits = 1 on logit 0 of every row unless stated.

    "tie"    : row 0's slots both hold o[0] = 2 (unit 0 ties at 2) and differ in coordinate 2 (5 against 7),
               which unit 0's W1 column ignores: gW1[2][0] is 5 if the lowest slot took the gradient, 7 if the
               highest did, 12 if both did. Rows 1 and 2 are empty sets.
    "masked" : row 0's slot 1 is masked and holds (inf, nan, nan, inf): its e would win. Slot 0 holds o[0] = 1.
    "empty"  : every row is an empty set; health 2, 3, 4.
    "nonpos" : every slot is live and every e is <= 0 (o[0] = -1 or 0, o[1] <= 1).
    "agents" : agents = (1, 0, 1); row 1's obs, health and dlogits are NaN and its mask is all ones."""
    E, N, S = 1, 3, 2
    obs = np.zeros((E, N, S, 4), F32)
    mask = np.zeros((E, N, S), np.uint8)
    health = np.ones((E, N), F64)
    dl = np.zeros((E, N, N_LOGITS), F32)
    dl[..., 0] = 1.0
    agents = None
    if name == "tie":
        obs[0, 0, 0] = (2, 0, 5, 1)
        obs[0, 0, 1] = (2, 0, 7, 3)
        mask[0, 0] = 1
    elif name == "masked":
        obs[0, 0, 0] = (1, 0, 3, 0)
        obs[0, 0, 1] = (np.inf, np.nan, np.nan, np.inf)
        mask[0, 0] = (1, 0)
    elif name == "empty":
        obs[:] = 9.0
        health[0] = (2, 3, 4)
    elif name == "nonpos":
        obs[0, :, :, 0] = ((-1, 0), (0, -1), (-1, -1))
        obs[0, :, :, 1] = ((1, 0), (-3, 1), (0.5, 1))
        obs[0, :, :, 2] = 4.0
        mask[:] = 1
    elif name == "agents":
        obs[0, 0, 0] = (3, 2, 1, 0)
        obs[0, 2, 1] = (1, 4, 2, 5)
        mask[0, 0] = (1, 0)
        mask[0, 2] = (0, 1)
        obs[0, 1], health[0, 1], dl[0, 1] = np.nan, np.nan, np.nan
        mask[0, 1] = 1
        agents = np.array([1, 0, 1], np.uint8)
    else:
        raise KeyError(name)
    return dict(params=selector_params(hidden), obs=obs, mask=mask, health=health, dlogits=dl, agents=agents)


CONSTRUCTED = ("tie", "masked", "empty", "nonpos", "agents")


def case_grad(c, hidden, **kw):
    return grad(c["params"], hidden, c["obs"], c["mask"], c["health"], c["dlogits"], c.get("agents"), **kw)
