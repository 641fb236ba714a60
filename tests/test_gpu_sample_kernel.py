"""The one-shot kernels of the in-launch Gumbel draw: macm_policy_noise against tests/sample_ref.py
(the words bit for bit, the noise within the bound and under the cap), macm_policy_flock_sampled
against macm_policy_flock given that noise (bit for bit, every net shape), the _at forms of both at a first_row
(the job's rows of a shard, up to the last row a 32-bit word names), and the distribution of the sampled
actions against the softmax of the stored logits."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import sample_ref as S
from guard_bands import Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.policy import MlpPolicy, gumbel_noise, sample_config  # noqa: E402

import ctypes  # noqa: E402

DEV = "cuda:0"
SEED = 0x1234_5678_9ABC_DEF0  # >= 2**32: both key words are in use
CARRY = 2**32 - 2             # with n_dec = 4: the decision index crosses the carry into hi32(d)


def noise_and_words(seed, decision, n_dec, rows, first_row=None):
    """macm_policy_noise (first_row given: macm_policy_noise_at) into guarded buffers; (noise float32
    [n_dec, rows, 9], words uint32 [n_dec, rows, 3, 4])"""
    gn, gw = Guarded((n_dec, rows, 9), torch.float32, DEV), Guarded((n_dec, rows, 3, 4), torch.int32, DEV)
    cfg = sample_config(seed, decision)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if first_row is None:
        _abi.check(_abi.lib().macm_policy_noise(ctypes.byref(cfg), n_dec, rows, p(gn.t), p(gw.t), stream),
                   "macm_policy_noise")
    else:
        _abi.check(_abi.lib().macm_policy_noise_at(ctypes.byref(cfg), first_row, n_dec, rows, p(gn.t), p(gw.t), stream),
                   "macm_policy_noise_at")
    torch.cuda.synchronize()
    assert gn.bands_intact() and gw.bands_intact(), "a store outside the noise or the words buffer"
    return gn.t.cpu().numpy(), gw.t.cpu().numpy().view(np.uint32)


def check_noise(got, want64):
    """|g_dev - g_ref64| <= 2**-24 |g_ref64| + 2**-50 for every element; returns how many elements are not
    bit-equal to float32(g_ref64)."""
    err = np.abs(got.astype(np.float64) - want64)
    bound = 2.0**-24 * np.abs(want64) + 2.0**-50
    worst = float((err / bound).max())
    assert (err <= bound).all(), f"worst error {worst:.3f} of the bound"
    return int((got.view(np.uint32) != want64.astype(np.float32).view(np.uint32)).sum()), worst


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_words_bit_for_bit(rows):
    noise, words = noise_and_words(SEED, CARRY, 4, rows)
    want = S.words(SEED, CARRY, 4, rows)
    assert np.array_equal(words, want), "the words of Philox4x32-10 over (r, lo32(d), hi32(d), h)"
    assert len(np.unique(words)) > words.size * 0.99
    n, _ = check_noise(noise.reshape(4, rows, 3, 3), S.gumbel64(want[..., :3]))
    assert n == 0, "on these few elements the device rounds as the reference does"
    # without the words (NULL) the noise is the same
    assert np.array_equal(gumbel_noise(SEED, CARRY, 4, (rows,), DEV).cpu().numpy().view(np.uint32), noise.view(np.uint32))


@pytest.mark.parametrize("first_row", [1, 63 * 64, 2**32 - 65], ids=["1", "63x64", "top"])
def test_words_at_a_first_row_bit_for_bit(first_row):
    """macm_policy_noise_at: row r draws as the job's row first_row + r, up to the last row a 32-bit word names
    (first_row + rows = 2**32: the word does not wrap)."""
    rows = 65
    noise, words = noise_and_words(SEED, CARRY, 4, rows, first_row)
    want = S.words(SEED, CARRY, 4, rows, first_row=first_row)
    assert np.array_equal(words, want), "the words of Philox4x32-10 over (first_row + r, lo32(d), hi32(d), h)"
    assert not np.array_equal(words, S.words(SEED, CARRY, 4, rows)), "first_row is part of the counter"
    n, _ = check_noise(noise.reshape(4, rows, 3, 3), S.gumbel64(want[..., :3]))
    assert n == 0, "on these few elements the device rounds as the reference does"
    # the Python helper, with and without the words
    g, w = gumbel_noise(SEED, CARRY, 4, (rows,), DEV, words=True, first_row=first_row)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(g.cpu().numpy().view(np.uint32), noise.view(np.uint32))
    assert np.array_equal(gumbel_noise(SEED, CARRY, 4, (rows,), DEV, first_row=first_row).cpu().numpy().view(np.uint32),
                          noise.view(np.uint32))
    if first_row + rows < 2**32:  # rows [first_row, first_row + rows) of the job's tensor
        whole = gumbel_noise(SEED, CARRY, 4, (first_row + rows,), DEV)[:, first_row:]
        assert np.array_equal(whole.cpu().numpy().view(np.uint32), noise.view(np.uint32))
    # first_row = 0 through the _at entry point is macm_policy_noise
    n0, w0 = noise_and_words(SEED, CARRY, 4, rows, 0)
    n1, w1 = noise_and_words(SEED, CARRY, 4, rows)
    assert np.array_equal(w0, w1) and np.array_equal(n0.view(np.uint32), n1.view(np.uint32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("first_row", [63 * 64, 2**32 - 257], ids=["63x64", "top"])
def test_flock_sampled_at_equals_flock_given_the_noise_at(first_row, dtype):
    """macm_policy_flock_sampled_at against macm_policy_flock given macm_policy_noise_at's rows, bit for bit."""
    od, rows, d = (4 if dtype == torch.float32 else 6), 257, CARRY + 1
    pol = seeded_policy(od, 32, 2)
    g = torch.Generator(device=DEV)
    g.manual_seed(rows)
    obs = ((torch.rand((rows, od), device=DEV, generator=g, dtype=torch.float64) * 2 - 1) * 3).to(dtype)
    noise = gumbel_noise(SEED, d, 1, (rows,), DEV, first_row=first_row)[0]
    assert np.array_equal(noise.cpu().numpy().view(np.uint32),
                          S.noise(SEED, d, 1, rows, first_row=first_row)[0].view(np.uint32)), "on these few elements"
    lg_a, lg_b = Guarded((rows, 9), torch.float32, DEV), Guarded((rows, 9), torch.float32, DEV)
    act_a, act_b = Guarded((rows, 3), torch.uint8, DEV), Guarded((rows, 3), torch.uint8, DEV)
    pol.act(obs, noise=noise, logits=lg_a.t, out=act_a.t)
    pol.act(obs, seed=SEED, decision=d, first_row=first_row, logits=lg_b.t, out=act_b.t)
    torch.cuda.synchronize()
    for x in (lg_a, lg_b, act_a, act_b):
        assert x.bands_intact()
    assert torch.equal(act_a.t, act_b.t), "the actions of macm_policy_flock given the noise of these rows"
    assert torch.equal(lg_a.t.view(torch.int32), lg_b.t.view(torch.int32))
    assert len(torch.unique(act_b.t)) == 3
    assert not torch.equal(pol.act(obs, seed=SEED, decision=d), act_b.t), "another first_row, another draw"
    with pytest.raises(ValueError, match="needs seed"):
        pol.act(obs, first_row=first_row)
    with pytest.raises(_abi.MacmError, match="first_row"):
        pol.act(obs, seed=SEED, decision=d, first_row=2**32 - rows + 1)


def test_small_seed_and_decision_zero():
    """A seed below 2**32 (key word 1 is zero) and d = 0: the other end of both ranges."""
    noise, words = noise_and_words(7, 0, 2, 65)
    assert np.array_equal(words, S.words(7, 0, 2, 65))
    assert not np.array_equal(words, S.words(7 + 2**32, 0, 2, 65)), "hi32(seed) is part of the key"


def test_noise_against_the_reference():
    """2**20 elements and a few more: every element within the bound, and at most 8 per 2**20 not bit-equal to
    float32 of the reference's float64 value. A cap, not a tolerance: a 1-ulp float64 log moves the value
    before its rounding by about 3 * 2**-52 max(1, |g|), which straddles a float32 boundary with probability
    about 2**-27 per binade of |g| down to the grid's 2**-31: 0.3 expected in 2**20."""
    n_dec, rows = 8, 14564
    noise, words = noise_and_words(SEED, 5, n_dec, rows)
    want_w = S.words(SEED, 5, n_dec, rows)
    assert np.array_equal(words, want_w)
    assert noise.size >= 2**20
    differ, worst = check_noise(noise.reshape(n_dec, rows, 3, 3), S.gumbel64(want_w[..., :3]))
    print(f"macm_policy_noise against sample_ref: {noise.size} elements, worst error {worst:.3f} of the bound, "
          f"{differ} not bit-equal to float32(g_ref64)")
    assert differ * 2**20 <= 8 * noise.size, f"{differ} elements differ in bits from float32(g_ref64)"
    assert np.isfinite(noise).all()
    # the first moments of Gumbel(0, 1): mean 0.5772, variance pi^2 / 6, to 6 sigma of their estimators
    n = noise.size
    assert abs(noise.astype(np.float64).mean() - 0.5772156649) < 6 * np.sqrt(np.pi**2 / 6 / n)
    # (the variance of a sample variance is (kurtosis - 1) sigma^4 / n, and Gumbel's kurtosis is 5.4)
    assert abs(noise.astype(np.float64).var() - np.pi**2 / 6) < 6 * np.sqrt(4.4 * (np.pi**2 / 6) ** 2 / n)


def seeded_policy(od, H, nh):
    pol = MlpPolicy(od, H, nh, DEV)
    pol.params.copy_(torch.from_numpy(pr.seeded_params(od, H, nh)))
    return pol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("od", [4, 6])
@pytest.mark.parametrize("H,nh", [(16, 1), (16, 2), (32, 1), (32, 2)])
def test_flock_sampled_equals_flock_given_the_noise(H, nh, od, dtype):
    pol = seeded_policy(od, H, nh)
    for rows, d in ((65, 0), (257, CARRY + 1)):
        g = torch.Generator(device=DEV)
        g.manual_seed(rows)
        obs = ((torch.rand((rows, od), device=DEV, generator=g, dtype=torch.float64) * 2 - 1) * 3).to(dtype)
        noise = gumbel_noise(SEED, d, 1, (rows,), DEV)[0]
        lg_a, lg_b = Guarded((rows, 9), torch.float32, DEV), Guarded((rows, 9), torch.float32, DEV)
        act_a, act_b = Guarded((rows, 3), torch.uint8, DEV), Guarded((rows, 3), torch.uint8, DEV)
        pol.act(obs, noise=noise, logits=lg_a.t, out=act_a.t)
        pol.act(obs, seed=SEED, decision=d, logits=lg_b.t, out=act_b.t)
        torch.cuda.synchronize()
        for x in (lg_a, lg_b, act_a, act_b):
            assert x.bands_intact()
        assert torch.equal(act_a.t, act_b.t), f"rows {rows}: the actions of macm_policy_flock given the noise"
        assert torch.equal(lg_a.t.view(torch.int32), lg_b.t.view(torch.int32)), f"rows {rows}: the logits"
        # and the definition: argmax(logits + noise of the reference), where the device's noise has its bits
        ref_noise = S.noise(SEED, d, 1, rows)[0]
        if np.array_equal(ref_noise.view(np.uint32), noise.cpu().numpy().view(np.uint32)):
            assert np.array_equal(act_b.t.cpu().numpy(), pr.actions_of(lg_b.t.cpu().numpy(), ref_noise))
        assert len(torch.unique(act_b.t)) == 3
        # another decision, another draw; without logits (NULL) the same actions
        other = pol.act(obs, seed=SEED, decision=d + 1)
        assert not torch.equal(other, act_b.t)
        assert torch.equal(pol.act(obs, seed=SEED, decision=d), act_b.t)


def test_flock_sampled_rows_follow_the_flat_index():
    """obs [E, N, od]: row r = e * N + i, whatever the leading shape."""
    pol = seeded_policy(4, 32, 2)
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    obs = torch.rand((5, 13, 4), device=DEV, generator=g) * 4 - 2
    a = pol.act(obs, seed=9, decision=4)
    assert a.shape == (5, 13, 3)
    assert torch.equal(a.view(-1, 3), pol.act(obs.view(-1, 4), seed=9, decision=4))
    assert torch.equal(a, pol.act(obs, noise=gumbel_noise(9, 4, 1, (5, 13), DEV)[0]))
    with pytest.raises(ValueError, match="exclude"):
        pol.act(obs, noise=gumbel_noise(9, 4, 1, (5, 13), DEV)[0], seed=9)


def test_distribution_on_the_device():
    """2**18 identical obs rows: the class counts of every head within 6 sigma of the float64 softmax of the
    stored logits. One log, a sign error or a word used twice does not pass this."""
    R = 2**18
    pol = seeded_policy(4, 32, 2)
    obs = torch.tensor([1.5, -0.7, 2.0, 0.4], device=DEV).repeat(R, 1).contiguous()
    lg = torch.empty((R, 9), dtype=torch.float32, device=DEV)
    act = pol.act(obs, seed=SEED, decision=3, logits=lg).cpu().numpy()
    lg = lg.cpu().numpy()
    assert (lg.view(np.uint32) == lg.view(np.uint32)[0]).all(), "identical rows give identical logits"
    z = lg[0].astype(np.float64).reshape(3, 3)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    for h in range(3):
        for c in range(3):
            n, mean, sd = int((act[:, h] == c).sum()), R * p[h, c], np.sqrt(R * p[h, c] * (1 - p[h, c]))
            print(f"head {h} class {c}: {n} of {R}, expected {mean:.1f} +- {sd:.1f}")
            assert abs(n - mean) <= 6 * sd, (h, c, n, mean, sd)
