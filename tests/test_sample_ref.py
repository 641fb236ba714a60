"""The reference of the in-launch Gumbel draw (tests/sample_ref.py) against what it is defined by:
the generator's known answers, a Python-int implementation, g = -log(-log(u)) evaluated with `decimal`
at 50 digits, the distribution of argmax(logits + g), and first_row: a shard's rows are the job's. No GPU."""
import decimal

import numpy as np
import pytest

import sample_ref as S

SEED = 0x1234_5678_9ABC_DEF0  # >= 2**32: both key words are in use


def test_known_answers():
    for ctr, key, want in S.KNOWN:
        assert S.philox_int(ctr, key) == want
        got = S.philox(*ctr, *key)
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want


def test_numpy_matches_python_ints():
    rng = np.random.default_rng(11)
    v = rng.integers(0, 2**32, size=(1000, 6), dtype=np.uint64)
    got = S.philox(*(v[:, i] for i in range(6)))
    for i in range(v.shape[0]):
        assert tuple(int(x) for x in got[i]) == S.philox_int(v[i, :4], v[i, 4:]), i


def test_words_follow_the_counter_layout():
    """counter = (r, lo32(d), hi32(d), h), key = (lo32(seed), hi32(seed)), across the carry into hi32(d)"""
    d0 = 2**32 - 2
    w = S.words(SEED, d0, 4, 5)
    assert w.shape == (4, 5, 3, 4)
    for j in range(4):
        d = d0 + j
        for r in (0, 4):
            for h in range(3):
                want = S.philox_int((r, d & S.MASK, d >> 32, h), (SEED & S.MASK, SEED >> 32))
                assert tuple(int(x) for x in w[j, r, h]) == want


def test_first_row_names_the_rows_of_the_job():
    """words(seed, d, n, rows, first_row=f) is rows [f, f + rows) of the job's words(seed, d, n, f + rows): a
    shard of a job draws the job's rows. So is the noise."""
    d0 = 2**32 - 2
    for f, rows in ((0, 5), (1, 65), (63 * 64, 65), (3 * 33, 2 * 33)):
        whole = S.words(SEED, d0, 4, f + rows)
        part = S.words(SEED, d0, 4, rows, first_row=f)
        assert part.shape == (4, rows, 3, 4) and np.array_equal(part, whole[:, f:]), (f, rows)
        assert f == 0 or not np.array_equal(part, whole[:, :rows]), "another row, another draw"
        assert np.array_equal(S.noise(SEED, d0, 4, rows, first_row=f).view(np.uint32),
                              S.noise(SEED, d0, 4, f + rows)[:, f:].view(np.uint32))
    assert np.array_equal(S.words(SEED, 3, 2, 7, first_row=0), S.words(SEED, 3, 2, 7))


def test_first_row_at_the_top_of_the_range():
    """first_row = 2**32 - rows: the last rows a 32-bit word can name, against the Python-int generator; the
    row word does not wrap, and one row more is refused."""
    rows, d0 = 65, 2**32 - 2
    f = 2**32 - rows
    w = S.words(SEED, d0, 4, rows, first_row=f)
    for j in range(4):
        d = d0 + j
        for r in (0, 1, rows - 2, rows - 1):
            for h in range(3):
                want = S.philox_int((f + r, d & S.MASK, d >> 32, h), (SEED & S.MASK, SEED >> 32))
                assert tuple(int(x) for x in w[j, r, h]) == want, (j, r, h)
    assert (f + rows - 1) == S.MASK
    assert not np.array_equal(w[:, -1], S.words(SEED, d0, 4, 1)[:, 0]), "row 2**32 - 1 is not row 0"
    assert S.words(SEED, d0, 1, 0, first_row=2**32).shape == (1, 0, 3, 4)
    for bad_f, bad_rows in ((f + 1, rows), (-1, rows), (2**32, 1)):
        with pytest.raises(ValueError, match="first_row"):
            S.words(SEED, d0, 1, bad_rows, first_row=bad_f)


def _exact_g(w: int) -> decimal.Decimal:
    u = (decimal.Decimal(int(w)) + decimal.Decimal("0.5")) / decimal.Decimal(2**32)
    return -(-u.ln()).ln()


def _words_checked():
    """At least 4,096 words: random ones, both ends of the range, and the 64 nearest u = 1/e on each side,
    where g crosses zero."""
    rng = np.random.default_rng(5)
    mid = int(np.floor(2.0**32 / np.e - 0.5))  # u(mid) <= 1/e < u(mid + 1)
    near = np.arange(mid - 63, mid + 65, dtype=np.uint64)
    ends = np.array([0, 1, 2, 2**32 - 3, 2**32 - 2, 2**32 - 1], dtype=np.uint64)
    return np.concatenate([near, ends, rng.integers(0, 2**32, size=4096, dtype=np.uint64)]).astype(np.uint32)


def test_g_against_decimal():
    """|g64 - exact| <= 2**-50 max(1, |g|) on every word checked; the float32 roundings that differ from the
    exact value's rounding are counted. Among the words nearest u = 1/e they are common and no defect: there
    |g| is a few 2**-32, its float32 spacing is below the 2**-53 that -log(u), a number near 1, is known to,
    and the definition is the float64 chain, not the exact value. Away from there the count is the
    reference's own share of the device test's cap of 8 per 2**20."""
    w = _words_checked()
    assert w.size >= 4096 + 128
    u = S.uniform(w)
    assert np.all((u > 0) & (u < 1))
    g64 = S.gumbel64(w)
    assert np.all(np.isfinite(g64))
    mid = int(np.floor(2.0**32 / np.e - 0.5))
    assert g64[63] <= 0 < g64[64] and int(w[63]) == mid  # the crossing is inside the near set
    worst, differ_near, differ = 0.0, 0, 0
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for i in range(w.size):
            ex = _exact_g(int(w[i]))
            assert decimal.Decimal(float(u[i])) == (decimal.Decimal(int(w[i])) + decimal.Decimal("0.5")) / 2**32
            err = abs(decimal.Decimal(float(g64[i])) - ex)
            bound = decimal.Decimal(2) ** -50 * max(decimal.Decimal(1), abs(ex))
            assert err <= bound, (int(w[i]), float(g64[i]), ex)
            worst = max(worst, float(err / bound))
            # the exact value rounds to the reference's float32 iff it lies between the midpoints around it
            g32 = np.float32(g64[i])
            lo = (decimal.Decimal(float(np.nextafter(g32, np.float32(-np.inf)))) + decimal.Decimal(float(g32))) / 2
            hi = (decimal.Decimal(float(np.nextafter(g32, np.float32(np.inf)))) + decimal.Decimal(float(g32))) / 2
            if i < 128:
                differ_near += not (lo <= ex <= hi)
            else:
                differ += not (lo <= ex <= hi)
    print(f"g64 against decimal: {w.size} words, worst error {worst:.3f} of the bound, "
          f"float32 roundings that differ from the exact value's: {differ_near} of the 128 nearest 1/e, "
          f"{differ} of the other {w.size - 128}")
    assert differ * 2**20 <= 8 * (w.size - 128)  # the device test's cap, scaled to this sample: none here


def test_distribution_of_the_argmax():
    """argmax(logits + g) over 2**18 rows samples softmax(logits): every class count of every head within
    6 sigma. One log, a sign error or a word used twice does not pass this."""
    R = 2**18
    logits = np.array([0.0, 1.0, -0.5], np.float32)
    p = np.exp(logits.astype(np.float64))
    p /= p.sum()
    g = S.noise(SEED, 3, 1, R)[0].reshape(R, 3, 3)
    z = (logits[None, None, :] + g).astype(np.float32)
    a = np.argmax(z, axis=-1)  # the lowest index on ties, as the definition
    for h in range(3):
        for c in range(3):
            n, mean, sd = int((a[:, h] == c).sum()), R * p[c], np.sqrt(R * p[c] * (1 - p[c]))
            assert abs(n - mean) <= 6 * sd, (h, c, n, mean, sd)
    # the three heads use different words: their actions are not one column three times
    assert (a[:, 0] != a[:, 1]).mean() > 0.3 and (a[:, 1] != a[:, 2]).mean() > 0.3


def test_noise_layout():
    """noise[..., 3h + c] is word c of head h; word 3 is unused; rows and decisions are independent axes."""
    w = S.words(SEED, 9, 2, 7)
    n = S.noise(SEED, 9, 2, 7)
    assert n.shape == (2, 7, 9) and n.dtype == np.float32
    for h in range(3):
        for c in range(3):
            assert np.array_equal(n[..., 3 * h + c], S.gumbel64(w[..., h, c]).astype(np.float32))
    assert np.array_equal(S.noise(SEED, 10, 1, 7)[0], n[1])
    assert np.array_equal(S.noise(SEED, 9, 2, 3), n[:, :3])
