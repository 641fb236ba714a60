"""The step's exact-arithmetic and wave primitives, one at a time, on the device.

The library's bit-exactness rests on a few small device functions that replace the compiler's
default lowering or a library call: rcp_rn, sqrt_rn, div_by_invariant, obs_sqrt
(csrc/flock_common.hpp), act_trig / macm_action_trig and obs_atan2 with its core / finish split
(csrc/macm_math.h), the DPP primitives wave_prefix_max, wave_prefix_sum, wave_max,
wave_pairwise_sum, block_pairwise_sum, and spill::block_scan_excl (csrc/flock_spill.hpp). The
parity tests feed them whatever a few hundred env-steps produce; here each gets the inputs at
which it can go wrong — mantissas next to a rounding boundary, atan2 ratios at the reduction
thresholds, angles beside a table entry, a maximum in lane 16 or 32, sums whose order matters —
through tests/probe/libmacm_probe.so: kernels that call one function each, compiled with the
product's flags (tests/probe/Makefile; built by __graft_entry__.py build()).

Every comparison is bitwise and every case asserts 0 mismatches, unless stated otherwise. The
float32 reference is numpy float64 arithmetic rounded to float32: for one division or one square
root of float32 inputs that is the correctly rounded float32 result (53 >= 2 * 24 + 2: the double
rounding is innocuous). The reference of act_trig and obs_atan2 is the host build of the same header
(tests/probe/libmacm_hostmath.so, from tools/trig_shim.c): DESIGN's "host and device builds are
bit-identical"; the host build against glibc is the CPU suite's job (tests/test_action_trig.py).
The exhaustive forms stay in tools/ (rcp_sqrt_gpu_check.hip, sqrt_gpu_check.hip,
trig_gpu_check.hip); this is the stratified subset that runs every time."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_action_trig import table_angles

pytestmark = pytest.mark.gpu

PROBE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe")
FLT_EPSILON = np.float32(2.0 ** -23)
P, S = ctypes.c_void_p, ctypes.c_size_t


def _load(name):
    path = os.path.join(PROBE_DIR, name)
    if not os.path.exists(path):
        pytest.fail(f"{path} is missing: build it with `make -C tests/probe` (python __graft_entry__.py build does)")
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def probe():
    lib = _load("libmacm_probe.so")
    for name, n_ptr, block in (("rcp_rn", 2, 0), ("sqrt_rn", 2, 0), ("obs_sqrt_f32", 2, 0), ("obs_sqrt_f64", 2, 0),
                               ("div_by_invariant", 3, 0), ("act_trig", 2, 0), ("obs_atan2", 3, 0),
                               ("obs_atan2_split_neg", 3, 0), ("wave_prefix_max", 2, 1), ("wave_prefix_sum", 2, 1),
                               ("wave_max", 2, 1), ("wave_pairwise_sum", 2, 1), ("block_pairwise_sum", 2, 1),
                               ("block_scan_excl", 3, 1)):
        fn = getattr(lib, "probe_" + name)
        fn.argtypes = [P] * n_ptr + [S] + [ctypes.c_int] * block
        fn.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def hostmath():
    lib = _load("libmacm_hostmath.so")
    lib.shim_action_trig_n.argtypes = [P, P, S]
    lib.shim_action_trig_n.restype = None
    lib.shim_obs_atan2_n.argtypes = [P, P, P, S]
    lib.shim_obs_atan2_n.restype = None
    return lib


def run(fn, ins, outs, n, *extra):
    """One probe call: numpy inputs to the device, outputs [(shape, numpy dtype)] back as numpy."""
    tin = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins]
    tout = [torch.from_numpy(np.zeros(shape, dt)).cuda() for shape, dt in outs]
    torch.cuda.synchronize()
    st = fn(*[P(t.data_ptr()) for t in tin + tout], S(n), *extra)
    assert st == 0, f"{fn.__name__}: HIP status {st}"
    res = [t.cpu().numpy() for t in tout]
    return res[0] if len(res) == 1 else res


def hexes(a):
    a = np.asarray(a)
    u = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
    v = np.atleast_1d(u).ravel()
    return "[" + " ".join(f"{int(w):#x}" for w in v[:8]) + (f" ... {v.size} values]" if v.size > 8 else "]")


def assert_same_bits(what, got, want, *inputs):
    """0 mismatches between got and want, bit for bit; prints the first offending inputs in hex."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    if bad.any():
        rows = np.unique(np.argwhere(bad)[:, 0])[:6]
        msg = "; ".join("in " + " ".join(hexes(x[i]) for x in inputs) + f" got {hexes(got[i])} want {hexes(want[i])}"
                        for i in rows)
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches of {bad.size}: {msg}")


# ---- float32 inputs ---------------------------------------------------------------------------------

EDGE_MANTISSAS = np.array(sorted({0, 1, 2, 3, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFD, 0x7FFFFE, 0x7FFFFF}
                                 | {1 << k for k in range(2, 23)} | {(1 << k) - 1 for k in range(2, 23)}), np.uint32)


def per_binade(e_lo, e_hi, rng):
    """For every binade 2^e, e_lo <= e <= e_hi: the edge mantissas and 4096 random ones (float32)."""
    out = []
    for e in range(e_lo, e_hi + 1):
        m = np.concatenate([EDGE_MANTISSAS, rng.integers(0, 1 << 23, 4096, dtype=np.uint32)])
        out.append((np.uint32(e + 127) << np.uint32(23)) | m)
    return np.concatenate(out).view(np.float32)


def all_floats(lo, hi):
    """Every float32 in [lo, hi), lo and hi positive."""
    a, b = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
    return np.arange(a, b, dtype=np.uint32).view(np.float32)


def f32_ordinal(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def neighbours(x, k):
    """The float32 values within k ulps of each x (2k + 1 per x, in order), across zero as well."""
    o = f32_ordinal(np.atleast_1d(np.asarray(x, np.float32)))[:, None] + np.arange(-k, k + 1)[None, :]
    bits = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)
    return bits.view(np.float32).ravel()


def sqrt_inputs(rng):
    return np.concatenate([per_binade(-48, 127, rng), all_floats(1.0, 4.0)])


def tiny_inputs(rng):
    """Below 2^-48: +0, the smallest and largest denormal, random denormals, binades 2^-126 .. 2^-49."""
    den = np.concatenate([[0, 1, 0x007FFFFF], rng.integers(1, 1 << 23, 4096)]).astype(np.uint32).view(np.float32)
    return np.concatenate([den, per_binade(-126, -49, rng)])


# ---- rcp_rn, sqrt_rn, obs_sqrt, div_by_invariant ------------------------------------------------------

@pytest.mark.parametrize("case", ["binades", "all_of_1_2"])
def test_rcp_rn(probe, case):
    """rcp_rn(x) == 1.0f / x on its documented domain [2^-23, 2^64] (Normalize: FLT_EPSILON <= len < 2^64)."""
    if case == "binades":
        x = np.concatenate([per_binade(-23, 63, np.random.default_rng(1)), np.array([2.0 ** 64], np.float32)])
    else:
        x = all_floats(1.0, 2.0)
    assert x.min() >= np.float32(2.0 ** -23) and x.max() <= np.float32(2.0 ** 64)
    want = (1.0 / x.astype(np.float64)).astype(np.float32)
    assert_same_bits("rcp_rn", run(probe.probe_rcp_rn, [x], [(x.shape, np.float32)], x.size), want, x)


@pytest.mark.parametrize("case", ["binades", "all_of_1_4"])
def test_sqrt_rn(probe, case):
    """sqrt_rn(x) == sqrtf(x) for x >= 2^-48 (sqrt's rounding pattern has a period of two binades)."""
    x = per_binade(-48, 127, np.random.default_rng(2)) if case == "binades" else all_floats(1.0, 4.0)
    want = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert_same_bits("sqrt_rn", run(probe.probe_sqrt_rn, [x], [(x.shape, np.float32)], x.size), want, x)


def test_sqrt_rn_below_domain_stays_below_epsilon(probe):
    """Below 2^-48 sqrtf(x) < FLT_EPSILON, and sqrt_rn only has to say the same, so that Normalize
    returns before it divides. A NaN fails the comparison: Normalize would go on and divide."""
    x = tiny_inputs(np.random.default_rng(3))
    assert (np.sqrt(x.astype(np.float64)) < FLT_EPSILON).all()
    got = run(probe.probe_sqrt_rn, [x], [(x.shape, np.float32)], x.size)
    bad = ~(got < FLT_EPSILON)
    assert not bad.any(), f"sqrt_rn >= FLT_EPSILON or NaN at {int(bad.sum())} inputs: {hexes(x[bad][:6])} -> {hexes(got[bad][:6])}"


@pytest.mark.parametrize("ot", ["f32", "f64"])
def test_obs_sqrt(probe, ot):
    """obs_sqrt<float> is (double)sqrtf(x) and must equal (float)sqrt((double)x); obs_sqrt<double> is
    sqrt((double)x). +0, denormals and +inf are real inputs (lanes >= N are infinitely far away)."""
    rng = np.random.default_rng(4)
    x = np.concatenate([sqrt_inputs(rng), tiny_inputs(rng), np.array([0.0, np.inf], np.float32)])
    want = np.sqrt(x.astype(np.float64))
    if ot == "f32":
        want = want.astype(np.float32).astype(np.float64)
    got = run(getattr(probe, "probe_obs_sqrt_" + ot), [x], [(x.shape, np.float64)], x.size)
    assert_same_bits(f"obs_sqrt<{ot}>", got, want, x)


def invariant_K(radius, density):
    """K = mA + mB of two equal bodies, inv_mass in float32 as capi_common.hpp fill_body_params derives it."""
    r, d = np.float32(radius), np.float32(density)
    mass = d * np.float32(3.14159265359) * r * r
    inv = np.float32(1.0) / mass
    return np.float32(inv + inv)


@pytest.mark.parametrize("case", ["configs", "all_of_one_binade"])
def test_div_by_invariant(probe, case):
    """div_by_invariant(n, K) == n / K, sign bit included, for n in {+0, -0} u [2^-40, 0.2f] (nothing
    above: n = -b2Clamp(0.2f * (sep + slop), -0.2f, 0)) and K of the default and 63 random configs.

    What this can and cannot tell apart: with both fma corrections removed it fails at a quarter of
    the inputs; with only the second one removed it passes, and no input of the domain would fail it:
    a host search (glibc fmaf) over every n of [2^-40, 0.2f] for each of these 64 K, and over every n
    of one binade for 12,000 more K mantissas, found the once-corrected quotient equal to n / K
    everywhere."""
    rng = np.random.default_rng(5)
    k_def = invariant_K(0.5, 1.0)
    assert abs(float(k_def) - 2.546479) < 1e-6
    top = np.float32(0.2)
    assert int(top.view(np.uint32)) == 0x3E4CCCCD
    if case == "configs":
        ks = np.array([k_def] + [invariant_K(r, d) for r, d in zip(rng.uniform(0.05, 2.05, 63), rng.uniform(0.1, 10.1, 63))])
        num = per_binade(-40, -3, rng)
        num = np.concatenate([np.array([0.0, -0.0], np.float32), num[num <= top], neighbours(top, 2)[:3]])
        n, K = np.tile(num, ks.size), np.repeat(ks, num.size)
    else:
        n = all_floats(2.0 ** -8, 2.0 ** -7)
        K = np.full(n.shape, k_def, np.float32)
    assert n.max() == top if case == "configs" else n.max() < top
    assert (K > 0).all()
    want = (n.astype(np.float64) / K.astype(np.float64)).astype(np.float32)
    got = run(probe.probe_div_by_invariant, [n, K], [(n.shape, np.float32)], n.size)
    assert_same_bits("div_by_invariant", got, want, n, K)


# ---- act_trig ---------------------------------------------------------------------------------------

def trig_inputs():
    rng = np.random.default_rng(6)
    table = np.array(table_angles(), np.float32)
    assert table.size == 17
    k_pi4 = (np.arange(-8, 9) * (np.pi / 4)).astype(np.float32)
    below_2_19 = np.nextafter(np.float32(2.0 ** 19), np.float32(0))
    mag = np.exp2(rng.uniform(-30, 19, 1_000_000)).astype(np.float32)
    mag = mag[mag < np.float32(2.0 ** 19)]
    a = np.concatenate([
        neighbours(table, 2),                                     # beside each table entry
        neighbours(k_pi4, 4),                                     # quadrant boundaries (k = 0: +-0 and denormals)
        np.array([0.0, -0.0], np.float32),
        neighbours([4.0, -4.0], 4),                               # the pair / two-reduction switch
        np.array([below_2_19, -below_2_19], np.float32),
        rng.uniform(-np.pi - 0.1, np.pi + 0.1, 1_000_000).astype(np.float32),
        mag * rng.choice(np.array([-1.0, 1.0], np.float32), mag.size),
    ])
    assert (np.abs(a) < np.float32(2.0 ** 19)).all()
    return a


def test_act_trig_equals_host_build(probe, hostmath):
    """|a| < 2^19: the device's four doubles are the host build's, bit for bit (sin(-0) = -0 included)."""
    a = trig_inputs()
    want = np.zeros((a.size, 4), np.float64)
    hostmath.shim_action_trig_n(P(a.ctypes.data), P(want.ctypes.data), S(a.size))
    got = run(probe.probe_act_trig, [a], [((a.size, 4), np.float64)], a.size)
    assert_same_bits("act_trig", got, want, a)


def test_act_trig_library_branch(probe):
    """|a| >= 2^19 (injected state only): the device libm. Its float64 results may be a few ulps from
    the true values, which moves a float32 rounding by at most one: the float32 roundings of the four
    results are within 1 float32 ulp of f32(mpmath sin / cos)."""
    import mpmath

    mags = np.array([2.0 ** 19, np.nextafter(np.float32(2.0 ** 19), np.float32(np.inf)), 2.0 ** 20 + 1, 1e9], np.float32)
    a = np.concatenate([mags, -mags])
    got = run(probe.probe_act_trig, [a], [((a.size, 4), np.float64)], a.size)
    want = np.zeros((a.size, 4), np.float32)
    with mpmath.workprec(200):
        for i, v in enumerate(a):
            x0, x1 = float(v), float(v) + np.pi / 2  # the second argument is a float64 sum, as in the step
            want[i] = [float(mpmath.sin(mpmath.mpf(x0))), float(mpmath.cos(mpmath.mpf(x0))),
                       float(mpmath.sin(mpmath.mpf(x1))), float(mpmath.cos(mpmath.mpf(x1)))]
    dist = np.abs(f32_ordinal(got.astype(np.float32)) - f32_ordinal(want))
    print("act_trig library branch, float32 ulps from mpmath:", dist.tolist())
    assert np.isfinite(got).all() and (dist <= 1).all(), f"inputs {hexes(a[(dist > 1).any(axis=1)])}: {dist.tolist()}"


# ---- obs_atan2 --------------------------------------------------------------------------------------

def quadrants(y, x):
    return (np.concatenate([y, y, -y, -y]), np.concatenate([x, -x, x, -x]))


def atan2_inputs():
    """(y, x) as float32-valued doubles (the observation's rel is float32)."""
    rng = np.random.default_rng(7)
    ys, xs = [], []

    def add(y, x, both_orders=False):
        y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
        qy, qx = quadrants(y, x)
        ys.append(qy)
        xs.append(qx)
        if both_orders:
            ys.append(qx)
            xs.append(qy)

    zero = np.zeros(1, np.float32)
    add(zero, zero)                                                     # the four signed-zero pairs
    mags = (np.uint32(127 - 126) + np.arange(0, 187, dtype=np.uint32))  # binades 2^-126 .. 2^60
    mags = np.concatenate([(mags << np.uint32(23)) | np.uint32(m) for m in (0, 0x400000, 0x7FFFFF)]).view(np.float32)
    add(np.zeros_like(mags), mags, both_orders=True)                    # both axes, with +-0 on the other
    add(mags, mags)                                                     # |y| = |x|
    # the reduction thresholds 7/16 and 11/16: random mx, and mx of <= 20 significant bits, for which
    # the threshold is a float32 and mn lies exactly on it
    e = rng.integers(-20, 21, 8192).astype(np.uint32) + np.uint32(127)
    m = rng.integers(0, 1 << 23, 8192, dtype=np.uint32)
    m[4096:] &= np.uint32(0x7FFFF0)
    mx = ((e << np.uint32(23)) | m).view(np.float32)
    for c in (0.4375, 0.6875):
        t = (c * mx.astype(np.float64)).astype(np.float32)
        assert (t[4096:].astype(np.float64) == c * mx[4096:].astype(np.float64)).all()
        add(neighbours(t, 2), np.repeat(mx, 5), both_orders=True)
    big = np.exp2(np.arange(-26, 61, 2)).astype(np.float32)             # ratios 2^-100 and 2^100
    add(big * np.float32(2.0 ** -100), big, both_orders=True)
    ys.append(rng.normal(0, 30, 1_000_000).astype(np.float32))         # the world's scale
    xs.append(rng.normal(0, 30, 1_000_000).astype(np.float32))
    y, x = np.concatenate(ys).astype(np.float64), np.concatenate(xs).astype(np.float64)
    assert np.isfinite(y).all() and np.isfinite(x).all()
    return y, x


def test_obs_atan2_equals_host_build_and_split(probe, hostmath):
    """obs_atan2 on the device == the host build of the same header, bit for bit; and, on the device
    alone, finish(core(|x|, |y|), -y, -x) == obs_atan2(-y, -x): the identity the TDM pair lanes use."""
    y, x = atan2_inputs()
    want = np.zeros_like(y)
    hostmath.shim_obs_atan2_n(P(y.ctypes.data), P(x.ctypes.data), P(want.ctypes.data), S(y.size))
    got = run(probe.probe_obs_atan2, [y, x], [(y.shape, np.float64)], y.size)
    assert_same_bits("obs_atan2", got, want, y, x)
    split = run(probe.probe_obs_atan2_split_neg, [y, x], [(y.shape, np.float64)], y.size)
    direct = run(probe.probe_obs_atan2, [-y, -x], [(y.shape, np.float64)], y.size)
    assert_same_bits("obs_atan2_finish(obs_atan2_core(|x|, |y|), -y, -x)", split, direct, y, x)


# ---- wave primitives --------------------------------------------------------------------------------

WAVE_BLOCKS = (64, 128, 1024)


def int_rows(rng, lo, hi, single):
    """[R, 64] int32 rows, R a multiple of 16 (whole blocks of 1024): 1024 random in [lo, hi), ascending,
    descending, all equal, and per lane p two rows whose single maximum / single nonzero is in lane p
    (the rest at their minimum, and the rest random below it): p = 15 / 16, 31 / 32, 47 / 48 are where
    the row shifts end and the two row broadcasts hand over."""
    rnd = rng.integers(lo, hi, (1024, 64))
    asc = np.sort(rng.integers(lo, hi, (8, 64)), axis=1)
    eq = np.repeat(rng.integers(lo, hi, (8, 1)), 64, axis=1)
    flat = np.full((64, 64), lo if single == "max" else 0)
    flat[np.arange(64), np.arange(64)] = hi - 1
    low = rng.integers(lo, (lo + hi) // 2, (64, 64)) if single == "max" else np.zeros((64, 64), np.int64)
    low[np.arange(64), np.arange(64)] = hi - 1 if single == "max" else 1
    rows = np.concatenate([rnd, asc, asc[:, ::-1], eq, flat, low])
    pad = -rows.shape[0] % 16
    return np.concatenate([rows, rng.integers(lo, hi, (pad, 64))]).astype(np.int32)


def report_rows(what, got, want, rows):
    got, want = got.reshape(rows.shape[0], -1), want.reshape(rows.shape[0], -1)
    bad = (got != want).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        at = np.flatnonzero(got[i] != want[i])[:8]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} rows differ; first row {i}, threads {at.tolist()}: "
                             f"got {hexes(got[i][at])} want {hexes(want[i][at])}; row " +
                             " ".join(f"{int(v):#x}" for v in rows[i][:128]))


@pytest.mark.parametrize("block", WAVE_BLOCKS)
def test_wave_prefix_max_and_wave_max(probe, block):
    rows = int_rows(np.random.default_rng(8), -(1 << 30) + 1, 1 << 30, "max")
    want = np.maximum.accumulate(rows, axis=1)
    got = run(probe.probe_wave_prefix_max, [rows], [(rows.shape, np.int32)], rows.size, block)
    report_rows(f"wave_prefix_max, block {block}", got, want, rows)
    got = run(probe.probe_wave_max, [rows], [(rows.shape, np.int32)], rows.size, block)
    report_rows(f"wave_max, block {block}", got, np.repeat(rows.max(axis=1, keepdims=True), 64, axis=1), rows)


@pytest.mark.parametrize("block", WAVE_BLOCKS)
def test_wave_prefix_sum(probe, block):
    rows = int_rows(np.random.default_rng(9), 0, 1 << 20, "sum")
    want = np.cumsum(rows, axis=1, dtype=np.int32)
    got = run(probe.probe_wave_prefix_sum, [rows], [(rows.shape, np.int32)], rows.size, block)
    report_rows(f"wave_prefix_sum, block {block}", got, want, rows)


# ---- the pairwise reward sum ------------------------------------------------------------------------

def rec(x):
    """tests/test_host_checks.py's recursive restatement of the device's order, over the rows of x."""
    n = x.shape[1]
    return x[:, 0] if n == 1 else rec(x[:, :n // 2]) + rec(x[:, n // 2:])


def left_to_right(x):
    acc = x[:, 0].copy()
    for j in range(1, x.shape[1]):
        acc = acc + x[:, j]
    return acc


def order_sensitive_rows(n_cols, rows=4096):
    """Rows of float64 values of mixed exponents: sums of them depend on the order (float32 rewards
    widened to float64 do not: 64 24-bit significands sum exactly)."""
    rng = np.random.default_rng(0)
    return rng.uniform(-1, 1, (rows, n_cols)) * np.exp2(rng.integers(-20, 21, (rows, n_cols)))


def assert_order_matters(x, want):
    differ = np.mean(want != left_to_right(x))
    assert differ > 0.5, f"the pairwise tree differs from a left-to-right sum in only {differ:.0%} of the rows"


@pytest.mark.parametrize("block", [64, 128, 192, 320, 1024])
def test_wave_pairwise_sum(probe, block):
    """Every lane of every wave holds rec() of its wave's 64 values, whatever the block's size."""
    x = order_sensitive_rows(64, 4320)  # 18 * 240 waves: whole blocks at every size (1, 2, 3, 5, 16 waves)
    want = rec(x)
    assert_order_matters(x, want)
    got = run(probe.probe_wave_pairwise_sum, [x], [(x.shape, np.float64)], x.size, block)
    assert_same_bits(f"wave_pairwise_sum, block {block}", got, np.repeat(want[:, None], 64, axis=1), x)


@pytest.mark.parametrize("block", [64, 128, 192, 320, 1024])
def test_block_pairwise_sum(probe, block):
    """Thread 0's result == rec() of the block's values padded with +0.0 to P = 64 * 2^ceil(log2(waves))
    (192: 3 -> 4 waves, 320: 5 -> 8)."""
    x = order_sensitive_rows(block)
    waves = block // 64
    width = 64 * (1 << (waves - 1).bit_length())
    assert width >= block and (width == block) == (waves & (waves - 1) == 0)
    want = rec(np.concatenate([x, np.zeros((x.shape[0], width - block))], axis=1))
    assert_order_matters(x, want)
    got = run(probe.probe_block_pairwise_sum, [x], [((x.shape[0],), np.float64)], x.size, block)
    assert_same_bits(f"block_pairwise_sum, block {block}", got, want, x)


# ---- spill::block_scan_excl -------------------------------------------------------------------------

@pytest.mark.parametrize("block", [64, 128, 320, 1024])
def test_block_scan_excl(probe, block):
    """Exclusive scan in thread order, and the block's total as every thread sees it."""
    rng = np.random.default_rng(10)
    last = np.zeros((1, block), np.int64)
    last[0, -1] = 1
    rows = np.concatenate([rng.integers(0, 2, (16, block)), rng.integers(0, 1001, (16, block)),
                           np.zeros((1, block), np.int64), last]).astype(np.int32)
    incl = np.cumsum(rows, axis=1, dtype=np.int32)
    excl, total = run(probe.probe_block_scan_excl, [rows], [(rows.shape, np.int32)] * 2, rows.size, block)
    report_rows(f"block_scan_excl, block {block}: exclusive scan", excl, incl - rows, rows)
    report_rows(f"block_scan_excl, block {block}: total", total, np.repeat(incl[:, -1:], block, axis=1), rows)
