"""The numpy statement of the TDM set policy (tests/tdm_policy_ref.py) against exact rational arithmetic,
its invariances (slot order, masked slots, the empty set), the action rule with the 2-way head, and
gym_macm.tdm_policy.TdmSetPolicy.torch_logits against a float64 numpy statement and under gradcheck.
No GPU: torch_logits takes a params tensor on the CPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import tdm_policy_ref as ref
from tdm_policy_ref import F32, N_LOGITS, same_bits


def to_f32(fr: Fraction) -> np.float32:
    """The exact rational rounded to nearest-even float32, in integer arithmetic (no overflow handling:
    the cases stay far below float32's largest value)."""
    n, d = fr.numerator, fr.denominator
    if n == 0:
        return F32(0.0)
    # exact rounding: scale to an integer with 24 significant bits by hand
    sign = -1 if n < 0 else 1
    n = abs(n)
    e = n.bit_length() - d.bit_length()
    # find e with 2^e <= n/d < 2^(e+1)
    if (n << max(0, -e)) < (d << max(0, e)):
        e -= 1
    shift = min(23 - e, 149)  # n/d * 2^shift in [2^23, 2^24); a denormal: the quantum is 2^-149
    num, den = (n << shift, d) if shift >= 0 else (n, d << -shift)
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    return F32(sign * np.ldexp(np.float64(q), -shift))


def frac_dense(W, b, x):
    """One layer over one row in exact arithmetic with the float32 rounding of every fmaf step."""
    out = []
    for j in range(W.shape[1]):
        acc = F32(b[j])
        for k in range(W.shape[0]):
            acc = to_f32(Fraction(float(W[k, j])) * Fraction(float(x[k])) + Fraction(float(acc)))
        out.append(acc)
    return np.array(out, F32)


def frac_logits(params, hidden, o, m, h):
    ws, bs = ref.split_params(params, hidden)
    g = np.zeros(hidden, F32)
    for k in range(len(m)):
        if m[k]:
            e = frac_dense(ws[0], bs[0], o[k].astype(F32))
            e = np.where(e > 0, e, F32(0))
            g = np.where(e > g, e, g)
    u = np.concatenate([g, [F32(h)]]).astype(F32)
    t = frac_dense(ws[1], bs[1], u)
    t = np.where(t > 0, t, F32(0)).astype(F32)
    return g, t, frac_dense(ws[2], bs[2], t)


def small_case(seed, N=4, hidden=16, rows=3):
    rng = np.random.default_rng(seed)
    obs = (rng.standard_normal((rows, N, N - 1, 4)) * 3).astype(F32)
    mask = (rng.random((rows, N, N - 1)) < 0.7).astype(np.uint8)
    health = rng.random((rows, N))
    return ref.seeded_params(hidden, seed=seed), obs, mask, health


def test_to_f32_rounds_to_nearest_even():
    for v in (1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 0.1, -0.1, 1e-40, 3.0e38, 2.0 ** -149, 2.0 ** -150 * 3):
        assert to_f32(Fraction(v)) == F32(v), v
    assert to_f32(Fraction(1) + Fraction(1, 2 ** 24)) == F32(1.0)  # a tie goes to the even neighbour
    assert to_f32(Fraction(1) + Fraction(3, 2 ** 24)) == F32(1.0 + 2.0 ** -22)


@pytest.mark.parametrize("hidden", [16, 32])
def test_reference_against_exact_arithmetic_every_layer(hidden):
    params, obs, mask, health = small_case(3, hidden=hidden, rows=2)
    lg = ref.logits_of(params, hidden, obs, mask, health)
    g_ref = ref.pooled(params, hidden, obs.reshape(-1, 3, 4), mask.reshape(-1, 3))
    ws, bs = ref.split_params(params, hidden)
    for r in range(obs.shape[0]):
        for i in range(obs.shape[1]):
            g, t, z = frac_logits(params, hidden, obs[r, i], mask[r, i], np.float64(health[r, i]).astype(F32))
            row = r * obs.shape[1] + i
            assert same_bits(g_ref[row], g).all(), "pool"
            u = np.concatenate([g_ref[row], [F32(health[r, i])]]).astype(F32)[None]
            assert same_bits(ref.relu(ref.dense(ws[1], bs[1], u))[0], t).all(), "trunk"
            assert same_bits(lg[r, i], z).all(), "head"


def test_slot_permutation_leaves_logits_bit_identical():
    params, obs, mask, health = small_case(5, N=7, hidden=32, rows=4)
    lg = ref.logits_of(params, 32, obs, mask, health)
    rng = np.random.default_rng(0)
    for _ in range(3):
        perm = rng.permutation(obs.shape[2])
        assert same_bits(ref.logits_of(params, 32, obs[:, :, perm], mask[:, :, perm], health), lg).all()


def test_all_masked_row_is_the_trunk_on_zero_and_health():
    params, obs, mask, health = small_case(6, hidden=16)
    mask[:] = 0
    lg = ref.logits_of(params, 16, obs, mask, health)
    ws, bs = ref.split_params(params, 16)
    u = np.concatenate([np.zeros((health.size, 16), F32), health.reshape(-1, 1).astype(F32)], axis=1)
    want = ref.dense(ws[2], bs[2], ref.relu(ref.dense(ws[1], bs[1], u)))
    assert same_bits(lg.reshape(-1, N_LOGITS), want).all()


def test_masked_slots_hold_anything():
    params, obs, mask, health = small_case(8, N=6, hidden=16)
    lg = ref.logits_of(params, 16, obs, mask, health)
    for junk in (np.nan, np.inf, -np.inf, -0.0, 1e38):
        o = obs.copy()
        o[mask == 0] = junk
        assert same_bits(ref.logits_of(params, 16, o, mask, health), lg).all(), junk
    assert not np.isnan(lg).any()


def test_action_rule_with_the_two_way_head():
    z = np.zeros(N_LOGITS, F32)
    assert ref.actions_of(z).tolist() == [0, 0, 0, 0], "ties: the lowest index"
    z = np.array([0, 1, 1, 3, 2, 1, -1, -2, -0.5, 1, 2], F32)
    assert ref.actions_of(z).tolist() == [1, 0, 2, 1]
    z[9:] = [np.nan, -5]
    assert ref.actions_of(z)[3] == 1, "a NaN is never chosen over a number"
    z[9:] = [np.nan, np.nan]
    assert ref.actions_of(z)[3] == 0
    z[9:] = [-np.inf, -np.inf]
    assert ref.actions_of(z)[3] == 0, "-inf is not > -inf"
    z = np.zeros(N_LOGITS, F32)
    noise = np.zeros(N_LOGITS, F32)
    noise[10] = 1e-3
    noise[8] = 1.0
    assert ref.actions_of(z, noise).tolist() == [0, 0, 2, 1]
    acts = ref.actions_of(np.random.default_rng(1).standard_normal((500, N_LOGITS)).astype(F32))
    assert acts[:, :3].max() == 2 and acts[:, 3].max() == 1, "the attack head has two choices"


def torch_case(seed, N=5, hidden=16, rows=3):
    from gym_macm.tdm_policy import TdmSetPolicy
    params, obs, mask, health = small_case(seed, N=N, hidden=hidden, rows=rows)
    mask[0, 0] = 0  # an empty set among the rows
    obs = obs.astype(np.float64)
    obs[mask == 0] = np.nan  # what a masked slot holds must not matter, nor poison a gradient
    pol = TdmSetPolicy.__new__(TdmSetPolicy)  # the layout only: no device
    pol.hidden, pol.shapes = hidden, ref.layer_shapes(hidden)
    return pol, params, obs, mask, health


@pytest.mark.parametrize("hidden", [16, 32])
def test_torch_logits_float64_against_numpy(hidden):
    pol, params, obs, mask, health = torch_case(9, hidden=hidden)
    got = pol.torch_logits(torch.from_numpy(obs), torch.from_numpy(mask), torch.from_numpy(health),
                           params=torch.from_numpy(params).double()).numpy()
    want = ref.logits_f64(params, hidden, obs, mask, health)
    assert got.shape == want.shape == health.shape + (N_LOGITS,)
    assert (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), np.abs(got - want).max()
    # and the float32 definition is the same function: within float32 rounding of the float64 statement
    lg = ref.logits_of(params, hidden, obs, mask, health)
    assert np.abs(lg - want).max() < 1e-3


def test_torch_logits_gradcheck():
    pol, params, obs, mask, health = torch_case(10, N=4, hidden=16, rows=2)
    P = torch.from_numpy(params).double().requires_grad_(True)
    o, m, h = torch.from_numpy(obs), torch.from_numpy(mask), torch.from_numpy(health)
    assert torch.autograd.gradcheck(lambda p: pol.torch_logits(o, m, h, params=p), (P,), eps=1e-6, atol=1e-5)
    pol.torch_logits(o, m, h, params=P).sum().backward()
    assert torch.isfinite(P.grad).all(), "a masked NaN slot reached the gradient"


def test_combat_case_ends_by_combat_with_terminal_health_off_init():
    """The premises of the device test's autoreset case (tdm_policy_ref.COMBAT_CASE), on the CPU."""
    from oracle import OracleTDM
    from parity import combat_bot

    from gym_macm.tdm_world import tdm_config
    c = ref.COMBAT_CASE
    teams, E, K = c["teams"], c["E"], c["K"]
    N = sum(teams)
    cfg = tdm_config(teams, obs_f64=True, **c["cfg"])
    orc = OracleTDM(cfg, E, c["seed"])
    agents = np.arange(N) < teams[0]
    noise = ref.gumbel_noise((K, E, N, N_LOGITS), c["noise_seed"])
    arows, results = ref.oracle_closed_loop(orc, combat_bot, ref.seeded_params(c["H"]), c["H"], agents, K, noise,
                                            cfg.init_health)
    ends = [(k, e) for k, r in enumerate(results) for e in np.flatnonzero(r["done"])]
    assert any(results[k]["winner"][e] >= 0 for k, e in ends), "no episode ended by combat"
    assert len({k for k, _ in ends}) > 1, "the episodes end at one step only"
    assert any((results[k]["health"][e, agents] != cfg.init_health).any() for k, e in ends), \
        "no reset env whose terminal health differs from init_health among the policy's agents"
    a = arows[1:, :, agents]
    assert set(np.unique(a[..., :3])) == {0, 1, 2} and set(np.unique(a[..., 3])) == {0, 1}, "the policy's decisions differ"


def mutant_mean_pool(params, hidden, obs, mask, health):
    ws, bs = ref.split_params(params, hidden)
    o, m = obs.reshape(-1, obs.shape[-2], 4), mask.reshape(-1, mask.shape[-1])
    e = np.stack([ref.relu(ref.dense(ws[0], bs[0], o[:, k].astype(F32))) for k in range(o.shape[1])], 1)
    e = np.where(m[..., None] != 0, e, 0)
    g = (e.sum(1) / np.maximum(m.sum(1), 1)[:, None]).astype(F32)
    u = np.concatenate([g, health.reshape(-1, 1).astype(F32)], 1)
    return ref.dense(ws[2], bs[2], ref.relu(ref.dense(ws[1], bs[1], u))).reshape(health.shape + (N_LOGITS,))


def mutant_health_first(params, hidden, obs, mask, health):
    ws, bs = ref.split_params(params, hidden)
    g = ref.pooled(params, hidden, obs.reshape(-1, obs.shape[-2], 4), mask.reshape(-1, mask.shape[-1]))
    u = np.concatenate([health.reshape(-1, 1).astype(F32), g], 1)
    return ref.dense(ws[2], bs[2], ref.relu(ref.dense(ws[1], bs[1], u))).reshape(health.shape + (N_LOGITS,))


def mutant_masked_included(params, hidden, obs, mask, health):
    return ref.logits_of(params, hidden, obs, np.ones_like(mask), health)


@pytest.mark.parametrize("mutant", [mutant_mean_pool, mutant_health_first, mutant_masked_included])
def test_a_mutated_definition_fails(mutant):
    params, obs, mask, health = small_case(12, N=6, hidden=16, rows=4)
    assert mask.min() == 0 and mask.sum(-1).max() >= 2
    lg = ref.logits_of(params, 16, obs, mask, health)
    assert not same_bits(mutant(params, 16, obs, mask, health), lg).all()
    assert np.abs(mutant(params, 16, obs, mask, health) - lg).max() > 1e-3, "the mutation is not a rounding matter"
