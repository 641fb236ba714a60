"""csrc/macm_math.h against its earlier forms, bit for bit, on the host.

obs_atan2 (the zero of the r0 case selected into the fmas' addends instead of multiplied in, the
hi / lo constants picked by integer masks and the division written out, both on the device only)
and macm_sincos_pair (quadrant signs as integer XORs) were rearranged to issue fewer instructions;
every rearrangement claims the same bits for every input the step can produce. tests/probe/macm_math_parent.h keeps the functions as they were,
verbatim; tests/probe/math_forms.c builds both for the host with gcc -ffp-contract=off (the build
tools/trig_check.c uses) and compares. The device build is compared with the host build of the
new header in tests/test_gpu_primitives.py and tests/test_gpu_f64_forms.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_action_trig import table_angles

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gym-macm_amd", "csrc")
PROBE = os.path.join(REPO, "tests", "probe")
P, S = ctypes.c_void_p, ctypes.c_size_t


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("forms") / "libforms.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-I", PROBE,
                    os.path.join(PROBE, "math_forms.c"), "-lm", "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.forms_atan2_n.argtypes = [P, P, S, P]
    lib.forms_atan2_n.restype = S
    lib.forms_trig_bits.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, P]
    lib.forms_trig_bits.restype = S
    lib.forms_trig_n.argtypes = [P, S, P]
    lib.forms_trig_n.restype = S
    lib.forms_parent_atan2_n.argtypes = [P, P, P, S]
    lib.forms_parent_atan2_n.restype = None
    lib.forms_obs_atan2_n.argtypes = [P, P, P, S]
    lib.forms_obs_atan2_n.restype = None
    return lib


def bits(x):
    return int(np.float32(x).view(np.uint32))


def neighbours32(v, k):
    """Each float32 of v with its k neighbours on both sides (by bit pattern; v nonnegative and finite)."""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.int64)
    w = (u[:, None] + np.arange(-k, k + 1)[None, :]).ravel()
    return w[(w >= 0) & (w < 0x7F800000)].astype(np.uint32).view(np.float32)


def check_atan2(forms, y, x, what):
    y = np.ascontiguousarray(np.asarray(y, np.float32).astype(np.float64))
    x = np.ascontiguousarray(np.asarray(x, np.float32).astype(np.float64))
    assert y.shape == x.shape and np.isfinite(y).all() and np.isfinite(x).all()
    first = ctypes.c_size_t(0)
    bad = forms.forms_atan2_n(P(y.ctypes.data), P(x.ctypes.data), S(y.size), ctypes.byref(first))
    i = first.value
    assert bad == 0, f"{what}: {bad} of {y.size} differ, first y={y[i].hex()} x={x[i].hex()}"


def four_quadrants(mn, mx):
    """(y, x) = (+-mn, +-mx) and (+-mx, +-mn): both octant orders, all four sign pairs."""
    ys, xs = [], []
    for a, b in ((mn, mx), (mx, mn)):
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                ys.append(np.float32(sy) * a)
                xs.append(np.float32(sx) * b)
    return np.concatenate(ys), np.concatenate(xs)


def test_atan2_random_pairs(forms):
    rng = np.random.default_rng(11)
    n = 10_000_000
    # half at the world's scale, half with exponents spread over 2^-60 .. 2^60
    y = rng.normal(0, 30, n).astype(np.float32)
    x = rng.normal(0, 30, n).astype(np.float32)
    h = n // 2
    y[h:] *= np.exp2(rng.integers(-60, 61, n - h)).astype(np.float32)
    x[h:] *= np.exp2(rng.integers(-60, 61, n - h)).astype(np.float32)
    check_atan2(forms, y, x, "random pairs")


def test_atan2_reduction_thresholds(forms):
    """mn at and +-1 ulp (here +-2) around 7/16 mx, 11/16 mx and mx: where r0 / r1 / neither change."""
    rng = np.random.default_rng(12)
    e = rng.integers(-40, 41, 16384).astype(np.uint32) + np.uint32(127)
    m = rng.integers(0, 1 << 23, 16384, dtype=np.uint32)
    m[8192:] &= np.uint32(0x7FFFF0)  # <= 20 significant bits: the threshold is then a float32, mn exactly on it
    mx = ((e << np.uint32(23)) | m).view(np.float32)
    for c in (0.4375, 0.6875, 1.0):
        t = (c * mx.astype(np.float64)).astype(np.float32)
        assert (t[8192:].astype(np.float64) == c * mx[8192:].astype(np.float64)).all()
        mn = neighbours32(t, 2)
        check_atan2(forms, *four_quadrants(mn, np.repeat(mx, 5)), f"mn around {c} mx")
    # 2 mn = mx exactly: the r1 numerator is an exact zero
    check_atan2(forms, *four_quadrants(mx * np.float32(0.5), mx), "mn = mx / 2")


def test_atan2_axes_zeros_and_magnitudes(forms):
    """Each axis with both signed zeros on the other, the four signed-zero pairs, and magnitudes from the
    smallest denormal 2^-149 to 2^127 against each other (ratios up to 2^276)."""
    mags = np.exp2(np.arange(-149, 128, dtype=np.float64)).astype(np.float32)
    assert mags[0] > 0 and np.isfinite(mags[-1])
    edge = np.concatenate([mags, neighbours32(mags[1:-1], 1), [np.finfo(np.float32).max]]).astype(np.float32)
    zero = np.zeros_like(edge)
    check_atan2(forms, *four_quadrants(zero, edge), "axes")
    z1 = np.zeros(1, np.float32)
    check_atan2(forms, *four_quadrants(z1, z1), "signed zeros")
    a, b = np.meshgrid(mags, mags)
    check_atan2(forms, *four_quadrants(a.ravel(), b.ravel()), "magnitude grid")
    check_atan2(forms, *four_quadrants(edge, edge), "|y| = |x|")


def check_trig_bits(forms, lo, hi, stride, what):
    first = ctypes.c_uint32(0)
    bad = forms.forms_trig_bits(lo, hi, stride, ctypes.byref(first))
    assert bad == 0, f"{what}: {bad} angles differ, first bits {first.value:#x} (or its negative)"


def test_trig_every_angle_near_pi(forms):
    """Every float32 in [3, pi] and [-pi, -3]: where the step's wrap hands angles over."""
    assert bits(np.pi) == 0x40490FDB
    check_trig_bits(forms, bits(3.0), bits(np.pi), 1, "[3, pi] and [-pi, -3]")


def test_trig_every_binade_below_four(forms):
    """2^16 mantissas in every binade of |a| < 4 (denormals and zero included), both signs."""
    check_trig_bits(forms, 0x55, bits(4.0) - 1, 1 << 7, "binades below 4, mantissa stride 2^7")
    check_trig_bits(forms, 0, 0, 1, "+-0")


def test_trig_table_entries_and_neighbours(forms):
    """The 17 entries of csrc/trig_fix.inc and their +-2 ulp neighbours; angles beyond 4 (injected
    state) take the two-reduction path, which did not change, and are compared all the same."""
    ang = np.array(table_angles(), np.float32)
    assert ang.size == 17
    a = neighbours32(np.abs(ang), 2)
    a = np.ascontiguousarray(np.concatenate([a, -a, [0.0, -0.0, 4.0, -4.0, 524287.0]]).astype(np.float32))
    first = ctypes.c_size_t(0)
    bad = forms.forms_trig_n(P(a.ctypes.data), S(a.size), ctypes.byref(first))
    assert bad == 0, f"{bad} of {a.size} differ, first {float(a[first.value]).hex()}"
