"""grad_ref (the numpy reference of macm_policy_grad / macm_value_grad) against torch.autograd on the CPU,
and the two kinds of test input: integer inputs on which every association gives the same float32 bits, and
float inputs with a bound that a correct float32 backward keeps and a wrong one breaks. No GPU."""
import numpy as np
import pytest
import torch

import grad_ref as gr
from policy_ref import F32, F64

NETS = ("policy", "critic")
CASES = [(net,) + s for net in NETS for s in gr.SHAPES]  # 16 shapes
ROWS = 1000


def torch_f64(params, in_dim, hidden, n_hidden, n_out, obs, dout):
    """(autograd's flat float64 gradient of sum(out * dout), torch's own float64 layer inputs)"""
    ws, bs = gr.split_params(np.asarray(params, F64), in_dim, hidden, n_hidden, n_out)
    tw = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    tb = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    a = torch.tensor(np.asarray(obs, F64).reshape(-1, in_dim))
    acts = [a]
    for l, (w, b) in enumerate(zip(tw, tb)):
        a = a @ w + b
        if l < len(tw) - 1:
            a = torch.relu(a)
            acts.append(a)
    (a * torch.tensor(np.asarray(dout, F64).reshape(a.shape))).sum().backward()
    g = np.concatenate([np.concatenate([w.grad.numpy().reshape(-1), b.grad.numpy()]) for w, b in zip(tw, tb)])
    return g, [t.detach().numpy() for t in acts]


@pytest.mark.parametrize("net,in_dim,hidden,n_hidden", CASES)
def test_backward_formulas_equal_autograd_f64(net, in_dim, hidden, n_hidden):
    n_out = gr.N_OUT[net]
    params, obs, dout = gr.float_inputs(net, in_dim, hidden, n_hidden, 257)
    want, acts = torch_f64(params, in_dim, hidden, n_hidden, n_out, obs, dout)
    ws, _ = gr.split_params(np.asarray(params, F64), in_dim, hidden, n_hidden, n_out)
    got = gr.backward(ws, acts, dout)  # fed torch's own float64 activations
    scale = gr.backward([np.abs(w) for w in ws], [np.abs(a) for a in acts], np.abs(np.asarray(dout, F64)))
    assert got.shape == want.shape == (gr.n_params(in_dim, hidden, n_hidden, n_out),)
    assert np.all(np.abs(got - want) <= 1e-12 * scale)
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("net,in_dim,hidden,n_hidden", CASES)
def test_integer_inputs_are_exact_in_float32(net, in_dim, hidden, n_hidden):
    n_out = gr.N_OUT[net]
    params, obs, dout = gr.integer_inputs(net, in_dim, hidden, n_hidden, ROWS)
    g, G = gr.grad(params, in_dim, hidden, n_hidden, n_out, obs, dout)
    assert G.max() < 2 ** 24
    acts = gr.activations(params, in_dim, hidden, n_hidden, n_out, obs)
    for frac in gr.live_fractions(acts):
        assert 0.25 <= frac <= 0.75, frac
    ws, _ = gr.split_params(params, in_dim, hidden, n_hidden, n_out)
    g32 = gr.backward(ws, acts, dout, F32)  # a plain float32 backward, numpy's association
    assert g32.dtype == F32 and np.array_equal(g32.astype(F64), g)
    assert np.array_equal(g, np.round(g)) and np.abs(g).max() > 0


@pytest.mark.parametrize("net,in_dim,hidden,n_hidden", CASES)
def test_float_bound_holds_for_float32_and_catches_a_transpose(net, in_dim, hidden, n_hidden):
    n_out = gr.N_OUT[net]
    params, obs, dout = gr.float_inputs(net, in_dim, hidden, n_hidden, ROWS)
    g, G = gr.grad(params, in_dim, hidden, n_hidden, n_out, obs, dout)
    bound = gr.tol(G, ROWS, hidden)
    assert np.all(bound[G > 0] > 0)
    acts = gr.activations(params, in_dim, hidden, n_hidden, n_out, obs)
    ws, _ = gr.split_params(params, in_dim, hidden, n_hidden, n_out)
    g32 = gr.backward(ws, acts, dout, F32).astype(F64)
    used = np.abs(g32 - g)[G > 0] / bound[G > 0]
    print(f"{net} {in_dim} {hidden} {n_hidden}: a plain float32 backward uses {used.max():.4f} of the bound")
    assert used.max() <= 1.0, used.max()
    if n_hidden == 2:  # a wrong backward (W2 transposed in the d chain) violates it
        bad = [w.copy() for w in ws]
        bad[1] = np.ascontiguousarray(ws[1].T)
        over = (np.abs(gr.backward(bad, acts, dout) - g)[G > 0] / bound[G > 0]).max()
        print(f"{net} {in_dim} {hidden} {n_hidden}: W2 transposed is at {over:.0f} times the bound")
        assert over > 1.0, over


def test_relu_derivative_is_zero_at_zero():
    """The mask is the stored activation's: a unit whose pre-activation is exactly 0 passes no gradient."""
    in_dim, hidden, n_hidden, n_out = 4, 16, 1, 1
    params = np.zeros(gr.n_params(in_dim, hidden, n_hidden, n_out), F32)
    ws, bs = gr.split_params(params, in_dim, hidden, n_hidden, n_out)
    ws[1][:] = 1.0  # the head sees every unit; W1 = 0 and b1 = 0: every pre-activation is +0
    obs = np.ones((3, in_dim), F32)
    g, _ = gr.grad(params, in_dim, hidden, n_hidden, n_out, obs, np.ones(3, F32))
    gw, gb = gr.split_params(g, in_dim, hidden, n_hidden, n_out)
    assert not gw[0].any() and not gb[0].any() and gb[1][0] == 3.0
