"""macm_policy_grad / macm_value_grad (csrc/policy_grad.hip) through the C-ABI against tests/grad_ref.py:
every supported shape of both nets with float32 and float64 obs; integer inputs, on which every association
of the sums gives the same float32 and the device must equal the reference exactly, at row counts around a
tile, over several waves and past the cap on the partials; float inputs within grad_ref.tol. In every call
obs and dout carry NaN rows after `rows` (a tail lane that read them would show as NaN), grad starts as NaN
(it is overwritten, not accumulated), and grad and the workspace sit between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grad_ref as gr
from guard_bands import Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import policy as P  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
NETS = ("policy", "critic")
TAIL = 70  # NaN rows behind the rows of a call: more than a tile
# past the cap: tiles 0, cap and 2 cap belong to wave 0, and the last tile holds one row
BIG = 2 * P.GRAD_TILE_ROWS * P.GRAD_MAX_PARTIALS + P.GRAD_TILE_ROWS + 1
ROWS = (1, 63, 64, 65, 257, 1000, BIG)
FLOAT_ROWS = (65, 1000)


def workspace_bytes(rows):
    n = ctypes.c_int64(-1)
    _abi.check(_abi.lib().macm_mlp_grad_workspace(rows, ctypes.byref(n)), "macm_mlp_grad_workspace")
    return n.value


def make_net(net, od, H, nh, params):
    m = (P.MlpPolicy if net == "policy" else P.MlpCritic)(od, H, nh, DEV)
    m.params.copy_(torch.from_numpy(np.ascontiguousarray(params, F32)))
    return m


def with_nan_tail(a, dtype):
    full = np.full((a.shape[0] + TAIL,) + a.shape[1:], np.nan, dtype)
    full[:a.shape[0]] = a
    return torch.from_numpy(full).to(DEV)


def run_grad(m, net, obs, dout, f64, rows=None, stream=None):
    """One call through the C-ABI into guarded buffers; the gradient as numpy"""
    rows = obs.shape[0] if rows is None else rows
    tobs, tdout = with_nan_tail(obs, F64 if f64 else F32), with_nan_tail(dout, F32)
    grad = Guarded((m.params.numel(),), torch.float32, DEV)
    grad.t.fill_(float("nan"))
    nbytes = workspace_bytes(rows)
    ws = Guarded((max(nbytes, 16),), torch.uint8, DEV)
    torch.cuda.synchronize()
    fn = getattr(_abi.lib(), "macm_policy_grad" if net == "policy" else "macm_value_grad")
    _abi.check(fn(ctypes.byref(m.struct()), ctypes.c_void_p(tobs.data_ptr()), 1 if f64 else 0, rows,
                  ctypes.c_void_p(tdout.data_ptr()), ctypes.c_void_p(grad.t.data_ptr()),
                  ctypes.c_void_p(ws.t.data_ptr()) if nbytes else None, nbytes,
                  ctypes.c_void_p(stream.cuda_stream) if stream is not None else None), "grad")
    torch.cuda.synchronize()
    assert grad.bands_intact(), "a store outside grad"
    assert ws.bands_intact(), "a store outside the workspace"
    return grad.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def integer_case(net, od, H, nh, rows):
    params, obs, dout = gr.integer_inputs(net, od, H, nh, rows)
    g, G = gr.grad(params, od, H, nh, gr.N_OUT[net], obs, dout)
    return params, obs, dout, g, G


@functools.lru_cache(maxsize=None)
def float_case(net, od, H, nh, rows):
    params, obs, dout = gr.float_inputs(net, od, H, nh, rows)
    g, G = gr.grad(params, od, H, nh, gr.N_OUT[net], obs, dout)
    return params, obs, dout, g, G


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", gr.SHAPES)
@pytest.mark.parametrize("net", NETS)
def test_integer_inputs_equal_the_reference(net, od, H, nh, f64, rows):
    params, obs, dout, g, G = integer_case(net, od, H, nh, rows)
    assert G.max() < 2 ** 24, "every partial sum is an exact float32 integer"
    got = run_grad(make_net(net, od, H, nh, params), net, obs, dout, f64)
    want = g.astype(F32)
    bad = np.argwhere(got != want)  # (a NaN differs from everything; the sign of a zero sum is left open)
    assert bad.size == 0, f"{net} OD {od} H {H} layers {nh} rows {rows}: {len(bad)} of {want.size} differ, first " \
                          f"at {bad[0][0]}: got {got[bad[0][0]]} want {want[bad[0][0]]}"
    if rows >= 63:
        assert np.count_nonzero(want) > want.size // 4, "the gradient is not trivially zero"


@pytest.mark.parametrize("rows", FLOAT_ROWS)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", gr.SHAPES)
@pytest.mark.parametrize("net", NETS)
def test_float_inputs_within_the_bound(net, od, H, nh, f64, rows):
    params, obs, dout, g, G = float_case(net, od, H, nh, rows)
    got = run_grad(make_net(net, od, H, nh, params), net, obs, dout, f64).astype(F64)
    bound = gr.tol(G, rows, H)
    used = np.abs(got - g)[G > 0] / bound[G > 0]
    print(f"{net} OD {od} H {H} layers {nh} rows {rows}: {used.max():.4f} of the bound")
    assert np.isfinite(got).all()
    assert used.max() <= 1.0, used.max()
    assert not got[G == 0].any()


@pytest.mark.parametrize("net", NETS)
def test_same_arguments_same_bits_on_any_stream(net):
    od, H, nh, rows = 6, 32, 2, 70001  # 1094 tiles: many waves in flight, none with the same timing twice
    params, obs, dout = gr.float_inputs(net, od, H, nh, rows)
    m = make_net(net, od, H, nh, params)
    a = run_grad(m, net, obs, dout, False)
    b = run_grad(m, net, obs, dout, False)
    c = run_grad(m, net, obs, dout, False, stream=torch.cuda.Stream(DEV))
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("net", NETS)
def test_zero_rows_writes_zeros(net):
    od, H, nh = 4, 16, 2
    params, obs, dout = gr.float_inputs(net, od, H, nh, 8)
    got = run_grad(make_net(net, od, H, nh, params), net, obs, dout, False, rows=0)  # no workspace: NULL, 0 bytes
    assert got.shape == (gr.n_params(od, H, nh, gr.N_OUT[net]),)
    assert np.array_equal(got.view(np.uint32), np.zeros(got.shape, np.uint32))
