"""tdm_grad_ref (the numpy reference of macm_tdm_policy_grad) on the CPU: against torch.autograd of
TdmSetPolicy.torch_logits in float64 on tie-free inputs, against answers worked out by hand, and on constructed
rows that pin the pool's rule (the lowest tied slot, masked slots, the empty set, units whose every e is <= 0,
skipped agents). Four wrong definitions must each fail at least one of the constructed checks."""
import numpy as np
import pytest
import torch

import tdm_grad_ref as tg
import tdm_policy_ref as tp
from gym_macm import tdm_policy as TP

F32, F64 = np.float32, np.float64
MUTANTS = dict(highest=dict(tie="highest"), every=dict(tie="all"), masked=dict(use_mask=False),
               no_health=dict(health_row=False))


def shell(hidden, params):
    """A TdmSetPolicy without its device allocation (its constructor needs a GPU): enough for torch_logits."""
    pol = TP.TdmSetPolicy.__new__(TP.TdmSetPolicy)
    pol.device, pol.hidden, pol.shapes = torch.device("cpu"), hidden, TP.layer_shapes(hidden)
    pol.params = torch.from_numpy(np.asarray(params, F32))
    return pol


@pytest.mark.parametrize("hidden,n_agents", [(16, 2), (16, 5), (32, 9), (32, 3)])
def test_against_autograd_of_torch_logits(hidden, n_agents):
    c = tg.float_inputs(hidden, n_agents, 7)
    obs = c["obs"].astype(F32)
    fwd = tg.forward_f64(c["params"], hidden, obs, c["mask"], c["health"])
    # tie-free: per (row, unit) the two largest live e differ unless the pool is 0, and no pre-activation is 0
    ws, bs = tg.split_params(c["params"], hidden)
    pre1 = fwd["o"] @ ws[0].astype(F64) + bs[0].astype(F64)
    assert (pre1[fwd["live"]] != 0).all()
    assert (fwd["u"] @ ws[1].astype(F64) + bs[1].astype(F64) != 0).all()
    top2 = np.sort(fwd["e"], axis=1)[:, -2:, :] if n_agents > 2 else None
    if top2 is not None:
        assert ((top2[:, 0] != top2[:, 1]) | (top2[:, 1] == 0)).all()
    assert (fwd["live"].sum(axis=1) == 0).any(), "an empty set among the rows"
    want = tg.backward(ws, fwd, c["dlogits"], tg.receivers(fwd))

    P64 = torch.from_numpy(c["params"].astype(F64)).requires_grad_()
    z = shell(hidden, c["params"]).torch_logits(torch.from_numpy(obs), torch.from_numpy(c["mask"]),
                                                torch.from_numpy(c["health"]), params=P64)
    (z * torch.from_numpy(c["dlogits"].astype(F64))).sum().backward()
    got = P64.grad.numpy()
    assert np.abs(want).max() > 0
    sl = tg.layer_slices(hidden)
    assert np.abs(want[sl["W1"]]).max() > 0
    assert (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), np.abs(got - want).max()


@pytest.mark.parametrize("hidden", [16, 32])
def test_known_answers_by_hand(hidden):
    """One row, two slots, selector_params: e_0 = (2, 0), e_1 = (1, 2), so g = (2, 2): unit 0's winner is slot
    0 and unit 1's is slot 1. health 3: t = (2, 2, 3.5, 0, ...). d3 = (1, 2, 0, ...): d2 = 3 on units 0..2,
    dg = 3 on units 0 and 1."""
    H = hidden
    obs = np.array([[[2, 0, 5, 1], [1, 3, 7, 3]]], F32)
    mask = np.ones((1, 2), np.uint8)
    dl = np.zeros((1, tg.N_LOGITS), F32)
    dl[0, :2] = (1, 2)
    g, G = tg.grad(tg.selector_params(H), H, obs, mask, np.array([3.0]), dl)
    sl = tg.layer_slices(H)
    W1, W2, W3 = g[sl["W1"]].reshape(4, H), g[sl["W2"]].reshape(H + 1, H), g[sl["W3"]].reshape(H, tg.N_LOGITS)
    wW1 = np.zeros((4, H))
    wW1[:, 0], wW1[:, 1] = (6, 0, 15, 3), (3, 9, 21, 9)
    wb1 = np.zeros(H)
    wb1[:2] = 3
    wW2 = np.zeros((H + 1, H))
    wW2[0, :3] = wW2[1, :3] = 6
    wW2[H, :3] = 9
    wb2 = np.zeros(H)
    wb2[:3] = 3
    wW3 = np.zeros((H, tg.N_LOGITS))
    wW3[0, :2] = wW3[1, :2] = (2, 4)
    wW3[2, :2] = (3.5, 7)
    assert np.array_equal(W1, wW1) and np.array_equal(g[sl["b1"]], wb1)
    assert np.array_equal(W2, wW2) and np.array_equal(g[sl["b2"]], wb2)
    assert np.array_equal(W3, wW3) and np.array_equal(g[sl["b3"]], dl[0].astype(F64))
    assert np.array_equal(G, np.abs(g)), "every term here is positive"


def constructed_failures(hidden, **kw):
    """The names of the constructed checks that a definition (the reference with **kw) fails."""
    H, bad = hidden, []
    sl = tg.layer_slices(H)
    parts = lambda g: (g[sl["W1"]].reshape(4, H), g[sl["b1"]], g[sl["W2"]].reshape(H + 1, H), g[sl["b2"]])

    with np.errstate(invalid="ignore", over="ignore"):
        g, _ = tg.case_grad(tg.constructed_case("tie", H), H, **kw)
    W1, b1, W2, b2 = parts(g)
    if not (W1[2, 0] == 5 and W1[3, 0] == 1 and W1[0, 0] == 2 and b1[0] == 1):
        bad.append("tie: the lowest tied slot takes the gradient, once")

    with np.errstate(invalid="ignore", over="ignore"):
        g, _ = tg.case_grad(tg.constructed_case("masked", H), H, **kw)
    W1, b1, W2, b2 = parts(g)
    if not (np.isfinite(g).all() and W1[0, 0] == 1 and W1[2, 0] == 3 and b1[0] == 1):
        bad.append("masked: a masked slot is never read")

    g, _ = tg.case_grad(tg.constructed_case("empty", H), H, **kw)
    W1, b1, W2, b2 = parts(g)
    if W1.any() or b1.any():
        bad.append("empty: no layer-1 contribution")
    if not (W2[H, 2] == 9 and b2[2] == 3 and not W2[:H].any()):
        bad.append("empty: the health row and gb2 are not zero")

    c = tg.constructed_case("nonpos", H)
    fwd = tg.forward(c["params"], H, c["obs"], c["mask"], c["health"])
    assert fwd["live"].all() and not fwd["g"].any()
    g, _ = tg.case_grad(c, H, **kw)
    W1, b1, W2, b2 = parts(g)
    if W1.any() or b1.any() or not b2[2] == 3:
        bad.append("nonpos: a unit whose every e is <= 0 has no winner")

    c = tg.constructed_case("agents", H)
    g, _ = tg.case_grad(c, H, **kw)
    keep = c["agents"].astype(bool)
    alone = dict(c, agents=None, **{k: c[k][:, keep] for k in ("obs", "mask", "health", "dlogits")})
    # (the kept rows alone: two rows of two slots each are no env of N = 3, which the reference does not mind)
    g2, _ = tg.grad(alone["params"], H, alone["obs"].reshape(-1, 2, 4), alone["mask"].reshape(-1, 2),
                    alone["health"].reshape(-1), alone["dlogits"].reshape(-1, tg.N_LOGITS), **kw)
    if not (np.isfinite(g).all() and np.array_equal(g, g2) and g[sl["W1"]].any()):
        bad.append("agents: a skipped row is not read")
    return bad


@pytest.mark.parametrize("hidden", [16, 32])
def test_constructed_rows_and_the_wrong_definitions(hidden):
    assert constructed_failures(hidden) == []
    for name, kw in MUTANTS.items():
        assert constructed_failures(hidden, **kw), f"the wrong definition '{name}' passes every constructed check"


def test_integer_inputs_stay_exact_in_float32():
    """The shapes tests/test_gpu_tdm_grad_kernel.py runs at its smaller row counts (it asserts the same at every
    one it uses): G below 2^24, ties between slots of different content, and a gradient that is not trivial."""
    for H, N, E in ((16, 3, 22), (32, 9, 8), (32, 33, 2)):
        c = tg.integer_inputs(H, N, E)
        g, G = tg.case_grad(c, H)
        assert G.max() < 2 ** 24
        assert np.array_equal(g, np.round(g))
        fwd = tg.forward(c["params"], H, c["obs"], c["mask"], c["health"])
        assert tg.tied_units(fwd) > 0
        assert (c["mask"].reshape(-1, N - 1).sum(axis=1) == 0).any()
        sl = tg.layer_slices(H)
        assert np.count_nonzero(g) > g.size // 8 and np.count_nonzero(g[sl["W1"]]) > 0
