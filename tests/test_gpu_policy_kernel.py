"""macm_policy_flock (csrc/policy.hip, policy_mlp.hpp) against tests/policy_ref.py: logits and actions
bit for bit, over every supported shape (hidden 16 / 32, one or two hidden layers, 4 or 6 inputs),
float32 and float64 obs, noise and logits given or NULL; 4096 random rows plus crafted ones (zeros,
-0, denormals, |x| up to 2^20), crafted weights (-0 everywhere, denormal weights, identical columns,
a NaN logit, a NaN hidden unit) and the row counts around a wave and a block. Every buffer the kernel
writes sits between guard bands."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import policy_ref as pr
from guard_bands import Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.policy import MlpPolicy  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
SHAPES = list(itertools.product((4, 6), (16, 32), (1, 2)))  # (OD, H, n_hidden)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rows_for(od):
    """float64 [4096 + crafted, od]: random rows over several magnitudes (not float32 values, so a
    float64 obs world's rounding is part of the test), then the crafted rows."""
    rng = np.random.default_rng(100 + od)
    x = rng.standard_normal((4096, od)) * 10.0 ** rng.integers(-3, 3, (4096, 1))
    d = 2.0 ** -149
    crafted = [np.zeros(od), np.full(od, -0.0), np.full(od, d), np.full(od, -d), np.arange(1, od + 1) * d * 1000,
               np.full(od, 2.0 ** 20), np.full(od, -(2.0 ** 20)), (-1.0) ** np.arange(od) * (2.0 ** 20 - 0.5),
               np.full(od, 2.0 ** -126 * (1 - 2.0 ** -30)),  # float64 between the largest subnormal and 2^-126
               np.full(od, 1 + 2.0 ** -24), np.full(od, 1 + 2.0 ** -24 + 2.0 ** -50)]  # a tie to even, and just above
    return np.concatenate([x, np.array(crafted)])


@functools.lru_cache(maxsize=None)
def noise_for(rows):
    n = pr.gumbel_noise((rows, 9), 17)
    n[3, 1] = np.nan  # NaN noise: that z is never chosen
    n[5, :] = np.inf
    return n


@functools.lru_cache(maxsize=None)
def reference(od, H, nh, f64):
    """(logits, actions without noise, actions with noise) of the seeded weights over rows_for(od)"""
    x = rows_for(od)
    x = x if f64 else x.astype(F32)
    lg = pr.logits_of(pr.seeded_params(od, H, nh), od, H, nh, x)
    return lg, pr.actions_of(lg), pr.actions_of(lg, noise_for(x.shape[0]))


def make_policy(od, H, nh, params):
    pol = MlpPolicy(od, H, nh, DEV)
    pol.params.copy_(torch.from_numpy(np.ascontiguousarray(params, F32)))
    return pol


def run_kernel(pol, x, noise, want_logits):
    """macm_policy_flock through the C-ABI into guarded buffers; (actions, logits or None) as numpy"""
    rows = x.shape[0]
    obs = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    act = Guarded((rows, 3), torch.uint8, DEV)
    lg = Guarded((rows, 9), torch.float32, DEV) if want_logits else None
    nz = torch.from_numpy(noise).to(DEV) if noise is not None else None
    L = _abi.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _abi.check(L.macm_policy_flock(ctypes.byref(pol.struct()), p(obs), 1 if x.dtype == np.float64 else 0, rows, p(nz),
                                   p(act.t), p(lg.t) if lg else None, None), "macm_policy_flock")
    torch.cuda.synchronize()
    assert act.bands_intact(), "a store outside the actions buffer"
    assert lg is None or lg.bands_intact(), "a store outside the logits buffer"
    return act.t.cpu().numpy(), (lg.t.cpu().numpy() if lg else None)


def assert_bits(got, want, what):
    bad = np.argwhere(~pr.same_bits(got, want))  # bit for bit; a NaN's sign and payload are left open
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} logits differ, first at {bad[0]}: " \
                          f"got {bits(got)[tuple(bad[0])]:#x} want {bits(want)[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("with_logits", [False, True], ids=["nologits", "logits"])
@pytest.mark.parametrize("with_noise", [False, True], ids=["argmax", "noise"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_random_and_crafted_rows(od, H, nh, f64, with_noise, with_logits):
    x = rows_for(od)
    x = x if f64 else x.astype(F32)
    lg_ref, a_plain, a_noise = reference(od, H, nh, f64)
    pol = make_policy(od, H, nh, pr.seeded_params(od, H, nh))
    act, lg = run_kernel(pol, x, noise_for(x.shape[0]) if with_noise else None, with_logits)
    if with_logits:
        assert_bits(lg, lg_ref, f"OD {od} H {H} layers {nh}")
    want = a_noise if with_noise else a_plain
    bad = np.argwhere(act != want)
    assert bad.size == 0, f"{len(bad)} actions differ, first at {bad[0]}"
    assert len(np.unique(want)) == 3, "the decisions differ among the rows"


@pytest.mark.parametrize("rows", [1, 63, 65, 257])
def test_row_counts_around_a_wave_and_a_block(rows):
    od, H, nh = 6, 32, 2
    x = rows_for(od)[:rows]
    lg_ref, a_plain, _ = reference(od, H, nh, True)
    pol = make_policy(od, H, nh, pr.seeded_params(od, H, nh))
    act, lg = run_kernel(pol, x, None, True)
    assert_bits(lg, lg_ref[:rows], f"{rows} rows")
    assert np.array_equal(act, a_plain[:rows])
    # MlpPolicy.act: the same through the Python layer, any leading shape
    obs = torch.from_numpy(x).to(DEV).view(1, rows, od)
    out_lg = torch.empty((1, rows, 9), dtype=torch.float32, device=DEV)
    a2 = pol.act(obs, logits=out_lg)
    assert a2.shape == (1, rows, 3) and np.array_equal(a2.cpu().numpy()[0], act)
    assert_bits(out_lg.cpu().numpy()[0], lg_ref[:rows], "MlpPolicy.act")


def crafted_params(kind, od, H, nh):
    shapes = pr.layer_shapes(od, H, nh)
    rng = np.random.default_rng(5)
    if kind == "negzero":
        # every hidden pre-activation is -0 (-0 * x + -0 with x >= 0): relu gives +0, and the logits are
        # -0 + 1 * +0 = +0; a relu that let -0 through would give -0 + 1 * -0 = -0
        ws = [np.full(s, -0.0, F32) for s in shapes[:-1]] + [np.ones(shapes[-1], F32)]
        bs = [np.full(o, -0.0, F32) for _, o in shapes]
    elif kind == "denormal":
        # denormal first-layer weights and biases; a second hidden layer of small integers keeps the tiny
        # values alive (denormal weights there would underflow every product); the head scales them up
        ws = [(rng.integers(-2000, 2000, shapes[0]) * 2.0 ** -149).astype(F32)]
        ws += [rng.integers(-8, 8, s).astype(F32) for s in shapes[1:-1]]
        ws.append((rng.integers(-8, 8, shapes[-1]) * 2.0 ** 100).astype(F32))
        bs = [(rng.integers(-50, 50, o) * 2.0 ** -149).astype(F32) for _, o in shapes]
    elif kind == "ties":  # identical columns in every layer: all 9 logits equal, row by row
        ws = [np.repeat((rng.standard_normal((i, 1)) / np.sqrt(i)).astype(F32), o, axis=1) for i, o in shapes]
        bs = [np.full(o, 0.25, F32) for _, o in shapes]
    elif kind == "nan":
        ws = [np.abs(rng.standard_normal(s) * 0.1).astype(F32) for s in shapes]
        bs = [np.full(o, 0.5, F32) for _, o in shapes]
        ws[0][0, 5], ws[0][1, 5] = np.inf, -np.inf  # hidden unit 5: inf - inf = NaN, relu: +0
        ws[-1][0, 4], ws[-1][1, 4] = np.inf, -np.inf  # logit 4: NaN (hidden 0 and 1 are positive)
        ws[-1][2, 7] = np.inf  # logit 7: +inf
    return pr.pack_params(ws, bs)


@pytest.mark.parametrize("kind", ["negzero", "denormal", "ties", "nan"])
@pytest.mark.parametrize("od,H,nh", SHAPES)
def test_crafted_weights(kind, od, H, nh):
    rng = np.random.default_rng(9)
    rows = 130
    x = np.abs(rng.standard_normal((rows, od))).astype(F32) + F32(0.5)  # positive inputs
    if kind == "denormal":
        x[::2] = (rng.integers(1, 1 << 20, (len(x[::2]), od)) * 2.0 ** -149).astype(F32)
        x[1::2] *= F32(2.0 ** 20)
    params = crafted_params(kind, od, H, nh)
    lg_ref = pr.logits_of(params, od, H, nh, x)
    noise = pr.gumbel_noise((rows, 9), 3)
    pol = make_policy(od, H, nh, params)
    for nz in (None, noise):
        act, lg = run_kernel(pol, x, nz, True)
        assert_bits(lg, lg_ref, kind)
        assert np.array_equal(act, pr.actions_of(lg_ref, nz)), kind
    if kind == "negzero":
        assert (bits(lg_ref) == 0).all(), "relu(-0) = +0, so the logits are +0, not -0"
    elif kind == "denormal":
        assert len(np.unique(bits(lg_ref))) > rows and np.isfinite(lg_ref).all()
    elif kind == "ties":
        assert (bits(lg_ref) == bits(lg_ref[:, :1])).all() and (pr.actions_of(lg_ref) == 0).all()
        assert len(np.unique(pr.actions_of(lg_ref, noise))) == 3, "the noise breaks the ties"
    else:
        assert np.isnan(lg_ref[:, 4]).all() and np.isposinf(lg_ref[:, 7]).all()
        a = pr.actions_of(lg_ref)
        assert (a[:, 1] != 1).all() and (a[:, 2] == 1).all(), "the NaN logit is never chosen; +inf is"
