"""tests/policy_ref.py, the numpy statement of the MLP policy (include/macm.h, macm_policy_mlp), without
a GPU: its float32 fma is exact (against fractions.Fraction, on random triples and on crafted
double-rounding cases), relu and the argmax follow the definition at -0, NaN and ties, and the oracle's
closed loop under it visits every action value, so the GPU tests that use the same weights compare
decisions that differ."""
from fractions import Fraction

import numpy as np

import policy_ref as pr
from gym_macm.settings import flockSettings, to_config
from oracle import OracleFlock

F32 = np.float32


def round_f32(fr):
    """The float32 nearest to the Fraction fr, ties to even (inf past the largest finite), exactly."""
    if fr == 0:
        return F32(0.0)
    sign, mag = (-1, -fr) if fr < 0 else (1, fr)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)  # the spacing of float32 at this magnitude (subnormals: 2^-149)
    n, rem = divmod(mag, q)
    n = int(n)
    if rem * 2 > q or (rem * 2 == q and n % 2 == 1):
        n += 1
    v = Fraction(n) * q
    if v >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(v))  # exact: v is a float32 value


def exact_fma(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def random_triples(n, rng):
    """Float32 triples whose product and addend are of comparable size more often than not (so the sum
    cancels and rounds), over many binades, with subnormals and exact ties among them."""
    ea = rng.integers(-40, 40, n)
    eb = rng.integers(-40, 40, n)
    a = (rng.uniform(1, 2, n) * 2.0 ** ea * rng.choice([-1, 1], n)).astype(F32)
    b = (rng.uniform(1, 2, n) * 2.0 ** eb * rng.choice([-1, 1], n)).astype(F32)
    ec = ea + eb + rng.integers(-30, 30, n)
    c = (rng.uniform(1, 2, n) * 2.0 ** ec * rng.choice([-1, 1], n)).astype(F32)
    # a quarter: short mantissas, so that a * b + c lands on float32 midpoints exactly (ties to even)
    short = rng.random(n) < 0.25
    a[short] = (np.round(a[short].astype(np.float64) / 2.0 ** ea[short] * 64) / 64 * 2.0 ** ea[short]).astype(F32)
    b[short] = (np.round(b[short].astype(np.float64) / 2.0 ** eb[short] * 64) / 64 * 2.0 ** eb[short]).astype(F32)
    # some subnormal results: scale everything down
    tiny = rng.random(n) < 0.1
    a[tiny] *= F32(2.0 ** -70)
    c[tiny] *= F32(2.0 ** -70)
    b[tiny] *= F32(2.0 ** -60)
    c[tiny] *= F32(2.0 ** -60)
    return a, b, c


def test_fma32_equals_the_exact_fma_on_random_triples():
    rng = np.random.default_rng(1)
    a, b, c = random_triples(10_000, rng)
    got = pr.fma32(a, b, c)
    want = np.array([exact_fma(x, y, z) for x, y, z in zip(a, b, c)], F32)
    bad = np.flatnonzero((bits(got) != bits(want)) & ~((got == 0) & (want == 0)))
    assert bad.size == 0, [(a[i].hex(), b[i].hex(), c[i].hex(), got[i].hex(), want[i].hex()) for i in bad[:5]]
    assert np.count_nonzero(np.abs(got) < 2.0 ** -126) > 50, "subnormal results among the cases"


def double_rounding_cases():
    """a * b is a float32 midpoint exactly (1 + 2^-i + 2^-(24 - i) + 2^-24, whose last bit is half a
    float32 ulp) and c moves the sum off it by far less than half a float64 ulp: the float64 sum rounds
    back onto the midpoint, and rounding that to float32 goes to even whatever c's sign was."""
    cases = []
    for i in range(1, 12):
        for scale in (1.0, 2.0 ** 20, 2.0 ** -20):
            for sa in (1.0, -1.0):
                a = F32(sa * (1 + 2.0 ** -i) * scale)
                b = F32(1 + 2.0 ** -(24 - i))
                for c in (2.0 ** -60, -2.0 ** -60, 2.0 ** -100, -2.0 ** -100, 2.0 ** -149, -2.0 ** -149):
                    cases.append((a, b, F32(c * scale if abs(c) > 2.0 ** -140 else c)))
    return [np.array(v, F32) for v in zip(*cases)]


def test_fma32_on_crafted_double_rounding_cases():
    a, b, c = double_rounding_cases()
    p = a.astype(np.float64) * b.astype(np.float64)
    s = p + c.astype(np.float64)
    assert np.array_equal(s, p), "the float64 sum lost c: the sum is within half a float64 ulp of the midpoint"
    got = pr.fma32(a, b, c)
    want = np.array([exact_fma(x, y, z) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(bits(got), bits(want))
    naive = s.astype(F32)
    assert np.count_nonzero(bits(naive) != bits(want)) >= len(a) // 3, "a plain float64 sum double-rounds these"


def test_fma32_special_values():
    def f(a, b, c):
        return pr.fma32(np.array([a], F32), np.array([b], F32), np.array([c], F32))

    inf, nan = np.inf, np.nan
    assert bits(f(3e38, 10, 0))[0] == bits(F32(inf))
    assert np.isnan(f(inf, 1, -inf))[0] and np.isnan(f(0, inf, 1))[0] and np.isnan(f(nan, 1, 1))[0]  # some NaN
    assert pr.same_bits(f(inf, 1, -inf), -f(nan, 1, 1)).all() and not pr.same_bits(F32(0.0), F32(-0.0)).any()
    assert bits(f(-0.0, 2, -0.0))[0] == 0x80000000  # -0 + -0
    assert bits(f(0.0, 2, -0.0))[0] == 0  # +0 + -0 = +0 to nearest
    d = 2.0 ** -149
    assert f(d, 1, d)[0] == F32(2.0 ** -148)  # denormals are kept
    assert f(2.0 ** -100, 2.0 ** -49, 0)[0] == F32(d)
    assert pr.fma32(F32(2), F32(3), F32(1)).shape == () and pr.fma32(F32(2), F32(3), F32(1)) == F32(7)


def test_relu_of_negative_zero_and_nan_is_positive_zero():
    v = np.array([-0.0, np.nan, -1.0, 0.0, 2.0 ** -149, 3.0, -np.inf, np.inf], F32)
    got = pr.relu(v)
    assert got.dtype == F32
    assert list(bits(got)) == list(bits(np.array([0, 0, 0, 0, 2.0 ** -149, 3, 0, np.inf], F32)))


def test_argmax_ties_nan_and_null_noise():
    lg = np.zeros((1, 9), F32)
    assert pr.actions_of(lg).tolist() == [[0, 0, 0]], "a tie: the lowest index"
    lg[0] = [1, 2, 2, 3, 3, 1, -1, -1, -0.5]
    assert pr.actions_of(lg).tolist() == [[1, 0, 2]]
    assert pr.actions_of(lg, None).tolist() == pr.actions_of(lg, np.zeros((1, 9), F32)).tolist()
    # +0 and -0 tie
    z = np.array([[-0.0, 0.0, 0.0, 0.0, -0.0, 0.0, 0, 0, 0]], F32)
    assert pr.actions_of(z).tolist() == [[0, 0, 0]]
    # a NaN is never chosen over a number, wherever it stands; all NaN: 0
    nan = np.nan
    z = np.array([[nan, -5, -7, 1, nan, 0.5, 2, 3, nan]], F32)
    assert pr.actions_of(z).tolist() == [[1, 0, 1]]
    assert pr.actions_of(np.full((1, 9), nan, F32)).tolist() == [[0, 0, 0]]
    # a NaN in the noise only: that z is NaN
    noise = np.array([[0, nan, 0, 0, 0, 0, 0, 0, 0]], F32)
    assert pr.actions_of(lg, noise).tolist() == [[2, 0, 2]]
    # -inf everywhere: nothing exceeds the start, 0
    assert pr.actions_of(np.full((1, 9), -np.inf, F32)).tolist() == [[0, 0, 0]]
    # the noise add is one float32 rounding
    big = np.array([[2.0 ** 24, 2.0 ** 24, 0, 0, 0, 0, 0, 0, 0]], F32)
    one = np.array([[0, 1, 0, 0, 0, 0, 0, 0, 0]], F32)
    assert pr.actions_of(big, one).tolist() == [[0, 0, 0]], "2^24 + 1 rounds to 2^24: still a tie"


def test_layer_is_the_k_ordered_chain():
    """One layer against the chain written out with exact_fma; the order matters for these values."""
    W = np.array([[2.0 ** 24], [1.0], [-(2.0 ** 24)], [1.0]], F32)
    b = np.array([0.0], F32)
    x = np.ones((1, 4), F32)
    acc = b[0]
    for k in range(4):
        acc = exact_fma(W[k, 0], x[0, k], acc)
    assert pr.dense(W, b, x)[0, 0] == acc == F32(1.0)  # ((2^24 + 1) -> 2^24, - 2^24 -> 0, + 1): 1, not 2
    params = pr.seeded_params(6, 16, 2)
    assert params.shape == (pr.n_params(6, 16, 2),) == (6 * 16 + 16 + 16 * 16 + 16 + 16 * 9 + 9,)
    obs = np.random.default_rng(3).standard_normal((5, 6))
    lg = pr.logits_of(params, 6, 16, 2, obs)  # float64 obs
    assert np.array_equal(bits(lg), bits(pr.logits_of(params, 6, 16, 2, obs.astype(F32)))), "float64 obs round to nearest"
    ws, bs = pr.split_params(params, 6, 16, 2)
    assert np.array_equal(pr.pack_params(ws, bs), params)


def test_reference_closed_loop_visits_every_action():
    """The oracle under policy_ref (E = 4, N = 8, 30 steps, the seeded weights and noise the GPU tests
    use): every head takes each of its three values in at least 10% of the agent-steps."""
    E, N, K, od, H, nh = 4, 8, 30, 4, 32, 2
    orc = OracleFlock(to_config(flockSettings(), N, 1, obs_f64=True), None, E, 42)
    params = pr.seeded_params(od, H, nh)
    noise = pr.gumbel_noise((K, E, N, 9), 5)
    arows, lrows, results = pr.oracle_closed_loop(orc, params, od, H, nh, K, noise)
    assert arows.shape == (K + 1, E, N, 3) and lrows.shape == (K, E, N, 9) and arows.dtype == np.uint8
    taken = arows[:K].reshape(-1, 3)
    for h in range(3):
        for c in range(3):
            frac = float(np.mean(taken[:, h] == c))
            assert frac >= 0.10, f"head {h} takes value {c} in {frac:.1%} of the agent-steps"
    # the logits decide too: without the noise a good part of the decisions stays the same
    same = float(np.mean(pr.actions_of(lrows) == arows[1:]))
    assert 0.4 < same < 0.95, same
    assert np.isfinite(lrows).all()
