"""tests/value_ref.py, the numpy statement of the critic (include/macm.h, macm_value_mlp) and of macm_gae,
without a GPU: the critic on a few rows against fractions.Fraction with one rounding per fma (as
test_policy_ref.py pins the actor), and GAE against the Fraction recursion on inputs where every operation
is exact, with a done row that cuts the recursion and the K = 1 case."""
from fractions import Fraction

import numpy as np
import pytest

import policy_ref as pr
import value_ref as vr
from test_policy_ref import bits, exact_fma

F32 = np.float32


def exact_value(params, od, H, nh, row):
    """V of one obs row: the chain written out with exact_fma, one rounding per step."""
    ws, bs = vr.split_params(params, od, H, nh)
    x = [F32(v) for v in row]
    for li, (W, b) in enumerate(zip(ws, bs)):
        y = []
        for j in range(W.shape[1]):
            acc = b[j]
            for k in range(W.shape[0]):
                acc = exact_fma(W[k, j], x[k], acc)
            if li < len(ws) - 1:
                acc = acc if acc > 0 else F32(0.0)
            y.append(acc)
        x = y
    assert len(x) == 1
    return x[0]


@pytest.mark.parametrize("od,H,nh", [(4, 16, 1), (6, 16, 2), (4, 32, 2), (6, 32, 1)])
def test_critic_equals_the_fraction_chain(od, H, nh):
    params = vr.seeded_params(od, H, nh)
    assert params.shape == (vr.n_params(od, H, nh),) == (od * H + H + (H * H + H) * (nh - 1) + H + 1,)
    rng = np.random.default_rng(od * 100 + H + nh)
    rows = rng.standard_normal((4, od)) * 10.0 ** rng.integers(-2, 2, (4, 1))  # float64: rounding is part of it
    rows = np.concatenate([rows, np.zeros((1, od)), np.full((1, od), 2.0 ** -149)])
    got = vr.value_of(params, od, H, nh, rows)
    assert got.shape == (6,) and got.dtype == F32
    want = np.array([exact_value(params, od, H, nh, r) for r in rows], F32)
    assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(bits(got))) > 3, "the rows give different values"
    assert vr.value_of(params, od, H, nh, rows.reshape(2, 3, od)).shape == (2, 3)


def test_critic_is_not_the_actor():
    assert not np.array_equal(vr.seeded_params(4, 32, 2)[:64], pr.seeded_params(4, 32, 2)[:64])
    assert vr.layer_shapes(6, 16, 2) == [(6, 16), (16, 16), (16, 1)]


def test_critic_relu_gives_positive_zero():
    """Every hidden pre-activation is -0: relu gives +0, and V = -0 + 1 * +0 = +0 (a relu that let -0
    through would give -0)."""
    od, H, nh = 4, 16, 2
    shapes = vr.layer_shapes(od, H, nh)
    ws = [np.full(s, -0.0, F32) for s in shapes[:-1]] + [np.ones(shapes[-1], F32)]
    bs = [np.full(o, -0.0, F32) for _, o in shapes]
    v = vr.value_of(pr.pack_params(ws, bs), od, H, nh, np.ones((3, od), F32))
    assert (bits(v) == 0).all()


def fraction_gae(reward, values, boot, done, gamma, lam):
    """The recursion in exact rational arithmetic (no rounding anywhere)."""
    K = len(reward)
    g, gl = Fraction(gamma), Fraction(gamma) * Fraction(lam)
    adv, ret, carry = [None] * K, [None] * K, Fraction(0)
    for k in range(K - 1, -1, -1):
        delta = g * Fraction(float(boot[k])) + Fraction(float(reward[k])) - Fraction(float(values[k]))
        adv[k] = delta if done[k] else gl * carry + delta
        ret[k] = adv[k] + Fraction(float(values[k]))
        carry = adv[k]
    return adv, ret


def exact_inputs(K, E, N, seed):
    """Small integer rewards and values: with gamma = lambda = 0.5 every intermediate is a multiple of
    4^-K below 2^8, far inside float32's 24 bits, so every float32 operation is exact."""
    rng = np.random.default_rng(seed)
    reward = rng.integers(-4, 5, (K, E, N)).astype(F32)
    values = rng.integers(-8, 9, (K, E, N)).astype(F32)
    boot = rng.integers(-8, 9, (K, E, N)).astype(F32)
    return reward, values, boot


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_gae_equals_the_fraction_recursion_where_every_operation_is_exact(K):
    E, N = 3, 4
    reward, values, boot = exact_inputs(K, E, N, K)
    done = (np.random.default_rng(50 + K).random((K, E)) < 0.3).astype(np.uint8)
    adv, ret = vr.gae(reward, values, boot, done, 0.5, 0.5)
    assert adv.dtype == ret.dtype == F32 and adv.shape == ret.shape == (K, E, N)
    for e in range(E):
        for n in range(N):
            wa, wr = fraction_gae(reward[:, e, n], values[:, e, n], boot[:, e, n], done[:, e], 0.5, 0.5)
            assert [Fraction(float(v)) for v in adv[:, e, n]] == wa, (e, n)
            assert [Fraction(float(v)) for v in ret[:, e, n]] == wr, (e, n)


def test_a_done_row_cuts_the_recursion():
    K, E, N = 6, 2, 3
    reward, values, boot = exact_inputs(K, E, N, 9)
    done = np.zeros((K, E), np.uint8)
    done[3, 0] = 1  # env 0 ends at step 3; env 1 never
    adv, _ = vr.gae(reward, values, boot, done, 0.5, 0.5)
    # rows 0..3 of env 0 are the GAE of the first four rows alone; rows 4, 5 those of a 2-row trajectory
    head, _ = vr.gae(reward[:4], values[:4], boot[:4], np.zeros((4, E), np.uint8), 0.5, 0.5)
    assert np.array_equal(bits(adv[:4, 0]), bits(head[:, 0]))
    assert not np.array_equal(bits(adv[:4, 1]), bits(head[:, 1])), "env 1 did not end: its recursion goes on"
    delta3 = F32(0.5) * boot[3, 0] + reward[3, 0] - values[3, 0]
    assert np.array_equal(adv[3, 0], delta3)
    # what comes after the cut does not reach the rows before it
    reward2 = reward.copy()
    reward2[4:, 0] += 3
    adv2, _ = vr.gae(reward2, values, boot, done, 0.5, 0.5)
    assert np.array_equal(bits(adv2[:4, 0]), bits(adv[:4, 0])) and not np.array_equal(adv2[4:, 0], adv[4:, 0])
    # any nonzero byte counts as done
    done[3, 0] = 0x80
    adv3, _ = vr.gae(reward, values, boot, done, 0.5, 0.5)
    assert np.array_equal(bits(adv3), bits(adv))


def test_one_step_advantage_is_delta():
    rng = np.random.default_rng(4)
    reward, values, boot = (rng.standard_normal((1, 3, 5)).astype(F32) for _ in range(3))
    for done in (0, 1):
        adv, ret = vr.gae(reward, values, boot, np.full((1, 3), done, np.uint8), 0.99, 0.95)
        delta = (pr.fma32(F32(0.99), boot, reward) - values).astype(F32)
        # done: delta itself; not done: fma(gl, +0, delta) = delta
        assert np.array_equal(bits(adv), bits(delta))
        assert np.array_equal(bits(ret), bits((delta + values).astype(F32)))


def test_gae_roundings_are_those_of_the_definition():
    """One fma, one subtraction, one fma, one add: checked against exact_fma on random float32 inputs."""
    rng = np.random.default_rng(6)
    K = 4
    reward, values, boot = (rng.standard_normal((K, 1, 6)).astype(F32) for _ in range(3))
    gamma, lam = F32(0.99), F32(0.95)
    gl = F32(gamma * lam)
    adv, ret = vr.gae(reward, values, boot, np.zeros((K, 1), np.uint8), gamma, lam)
    for n in range(6):
        carry = F32(0.0)
        for k in range(K - 1, -1, -1):
            delta = F32(exact_fma(gamma, boot[k, 0, n], reward[k, 0, n]) - values[k, 0, n])
            a = exact_fma(gl, carry, delta)
            assert bits(adv[k, 0, n]) == bits(a) and bits(ret[k, 0, n]) == bits(F32(a + values[k, 0, n]))
            carry = a
