"""macm_value_flock (csrc/policy.hip, policy_mlp.hpp) against tests/value_ref.py, bit for bit: every
supported shape (hidden 16 / 32, one or two hidden layers, 4 or 6 inputs), float32 and float64 obs, the
row counts around a wave and a block, and rows that hold +-0, denormals, +-inf and NaN. The values buffer
sits between guard bands."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import policy_ref as pr
import value_ref as vr
from guard_bands import FILL, Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.policy import MlpCritic  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
SHAPES = list(itertools.product((4, 6), (16, 32), (1, 2)))  # (OD, H, n_hidden)
ROWS = (1, 63, 255, 257, 1000)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rows_for(od):
    """float64 [1000, od]: the crafted rows first (so that every row count holds some), then random rows
    over several magnitudes (not float32 values: a float64 obs world's rounding is part of the test)."""
    rng = np.random.default_rng(200 + od)
    d = 2.0 ** -149
    crafted = [np.zeros(od), np.full(od, -0.0), np.full(od, d), np.full(od, -d), np.arange(1, od + 1) * d * 1000,
               np.full(od, 2.0 ** -126 * (1 - 2.0 ** -30)), np.full(od, 1 + 2.0 ** -24), np.full(od, 2.0 ** 20)]
    x = rng.standard_normal((1000 - len(crafted), od)) * 10.0 ** rng.integers(-3, 3, (1000 - len(crafted), 1))
    return np.concatenate([np.array(crafted), x])


@functools.lru_cache(maxsize=None)
def reference(od, H, nh, f64):
    x = rows_for(od)
    return vr.value_of(vr.seeded_params(od, H, nh), od, H, nh, x if f64 else x.astype(F32))


def make_critic(od, H, nh, params):
    c = MlpCritic(od, H, nh, DEV)
    c.params.copy_(torch.from_numpy(np.ascontiguousarray(params, F32)))
    return c


def run_kernel(crit, x, rows=None):
    """macm_value_flock through the C-ABI into a guarded buffer; the values as numpy"""
    rows = x.shape[0] if rows is None else rows
    obs = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    val = Guarded((max(rows, 1),), torch.float32, DEV)
    _abi.check(_abi.lib().macm_value_flock(ctypes.byref(crit.struct()), ctypes.c_void_p(obs.data_ptr()),
                                           1 if x.dtype == np.float64 else 0, rows, ctypes.c_void_p(val.t.data_ptr()),
                                           None), "macm_value_flock")
    torch.cuda.synchronize()
    assert val.bands_intact(), "a store outside the values buffer"
    return val


def assert_bits(got, want, what):
    bad = np.argwhere(~pr.same_bits(got, want))  # bit for bit; a NaN's sign and payload are left open
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} values differ, first at {bad[0]}: " \
                          f"got {bits(got)[tuple(bad[0])]:#x} want {bits(want)[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_every_shape_and_row_count(od, H, nh, f64, rows):
    x = rows_for(od)[:rows]
    x = x if f64 else x.astype(F32)
    crit = make_critic(od, H, nh, vr.seeded_params(od, H, nh))
    got = run_kernel(crit, x).t.cpu().numpy()
    want = reference(od, H, nh, f64)[:rows]
    assert_bits(got, want, f"OD {od} H {H} layers {nh} rows {rows}")
    if rows >= 63:
        assert len(np.unique(bits(want))) > rows // 2, "the rows give different values"


def test_the_python_layer_any_leading_shape():
    od, H, nh = 6, 32, 2
    crit = make_critic(od, H, nh, vr.seeded_params(od, H, nh))
    x = rows_for(od)[:255]
    obs = torch.from_numpy(x).to(DEV).view(5, 51, od)
    v = crit.value(obs)
    assert v.shape == (5, 51) and v.dtype == torch.float32
    assert_bits(v.cpu().numpy().reshape(-1), reference(od, H, nh, True)[:255], "MlpCritic.value")
    out = torch.empty((5, 51), dtype=torch.float32, device=DEV)
    assert crit.value(obs, out=out) is out and torch.equal(out.view(torch.int32), v.view(torch.int32))
    with pytest.raises(ValueError, match="obs rows"):
        crit.value(obs.view(5, 102, 3).contiguous())
    with pytest.raises(ValueError, match="out must"):
        crit.value(obs, out=torch.empty((5, 50), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="obs must"):
        crit.value(obs.cpu())
    # from_linear_layers transposes [out, in] to [in][out]; unpack gives the layers back
    layers = [torch.nn.Linear(i, o) for i, o in vr.layer_shapes(od, H, nh)]
    ws, bs = vr.split_params(vr.seeded_params(od, H, nh), od, H, nh)
    with torch.no_grad():
        for lin, w, b in zip(layers, ws, bs):
            lin.weight.copy_(torch.from_numpy(w.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
    c2 = MlpCritic.from_linear_layers(layers, device=DEV)
    assert np.array_equal(c2.params.cpu().numpy(), vr.seeded_params(od, H, nh))
    uw, ub = c2.unpack()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(uw + ub, ws + bs))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_rows_with_zeros_denormals_infinities_and_nan(od, H, nh, f64):
    rng = np.random.default_rng(31)
    rows = 70
    x = rng.standard_normal((rows, od))
    d = 2.0 ** -149
    x[0] = 0.0
    x[1] = -0.0
    x[2] = d
    x[3] = -d
    x[4, 0], x[5, 1], x[6, 2] = np.inf, -np.inf, np.nan
    x[7] = np.inf
    x[8] = np.nan
    x[9, 0], x[9, 1] = np.inf, -np.inf
    x[10] = np.arange(1, od + 1) * d * 3
    x = x if f64 else x.astype(F32)
    params = vr.seeded_params(od, H, nh)
    crit = make_critic(od, H, nh, params)
    got = run_kernel(crit, x).t.cpu().numpy()
    want = vr.value_of(params, od, H, nh, x)
    assert_bits(got, want, "special rows")
    assert np.isfinite(want[:4]).all() and np.isfinite(want[10])
    if nh == 1:  # (two hidden layers: inf - inf = NaN in the second, which relu turns into +0)
        assert not np.isfinite(want[4:6]).any(), "one hidden layer: an infinite input reaches the output"
    # denormal weights keep denormal values alive: V is a denormal, not flushed to zero
    shapes = vr.layer_shapes(od, H, nh)
    ws = [np.full(shapes[0], d, F32)] + [np.eye(*s, dtype=F32) for s in shapes[1:]]
    bs = [np.zeros(o, F32) for _, o in shapes]
    dparams = pr.pack_params(ws, bs)
    xs = np.ones((3, od)) if f64 else np.ones((3, od), F32)
    got = run_kernel(make_critic(od, H, nh, dparams), xs).t.cpu().numpy()
    assert_bits(got, vr.value_of(dparams, od, H, nh, xs), "denormal weights")
    assert (bits(got) == od).all(), "od denormal steps: the value is od * 2^-149"


def test_zero_rows_writes_nothing():
    crit = make_critic(4, 32, 2, vr.seeded_params(4, 32, 2))
    val = run_kernel(crit, rows_for(4)[:8].astype(F32), rows=0)
    assert bool((val.raw == FILL).all())
