"""macm_gae (csrc/policy.hip, gae_kernel) against tests/value_ref.py, bit for bit: the shapes around a
wave, a block and the kernel's row chunk, four (gamma, lambda) pairs, five done patterns, a done byte other
than 0 or 1, and NaN / inf inputs. adv and ret sit between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import policy_ref as pr
import value_ref as vr
from guard_bands import FILL, Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.policy import gae  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
SHAPES = [(1, 3, 5), (2, 5, 64), (17, 9, 31), (40, 8, 64), (5, 1, 1)]
COEFS = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.0), (0.5, 0.0)]
PATTERNS = ["none", "all", "random", "row0", "last"]


def done_pattern(kind, K, E):
    d = np.zeros((K, E), np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "random":
        d = (np.random.default_rng([K, E, 71]).random((K, E)) < 0.3).astype(np.uint8)  # (71: true of every shape here)
        assert d.any() and not d.all(), "the seeded pattern holds both values"
    elif kind == "row0":
        d[0] = 1
    elif kind == "last":
        d[K - 1] = 1
    return d


@functools.lru_cache(maxsize=None)
def inputs(K, E, N):
    rng = np.random.default_rng([K, E, N])
    reward = rng.standard_normal((K, E, N)).astype(F32)
    values = (rng.standard_normal((K, E, N)) * 3).astype(F32)
    boot = (rng.standard_normal((K, E, N)) * 3).astype(F32)
    return reward, values, boot


def run_kernel(reward, values, boot, done, gamma, lam):
    K, E, N = reward.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    r, v, b, d = t(reward), t(values), t(boot), t(done)
    adv, ret = Guarded((K, E, N), torch.float32, DEV), Guarded((K, E, N), torch.float32, DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    _abi.check(_abi.lib().macm_gae(p(r), p(v), p(b), p(d), K, E, N, gamma, lam, p(adv.t), p(ret.t), None), "macm_gae")
    torch.cuda.synchronize()
    assert adv.bands_intact() and ret.bands_intact(), "a store outside adv / ret"
    for name, x, a in (("reward", r, reward), ("values", v, values), ("boot", b, boot), ("done", d, done)):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), f"{name} was written"
    return adv.t.cpu().numpy(), ret.t.cpu().numpy()


def assert_bits(got, want, what):
    bad = np.argwhere(~pr.same_bits(got, want))
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[0]}: " \
                          f"got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("gamma,lam", COEFS)
@pytest.mark.parametrize("K,E,N", SHAPES)
def test_gae_equals_the_reference(K, E, N, gamma, lam, pattern):
    reward, values, boot = inputs(K, E, N)
    done = done_pattern(pattern, K, E)
    adv, ret = run_kernel(reward, values, boot, done, gamma, lam)
    wadv, wret = vr.gae(reward, values, boot, done, gamma, lam)
    assert_bits(adv, wadv, "adv")
    assert_bits(ret, wret, "ret")
    if K >= 17 and pattern == "none" and gamma == 0.99:
        one, _ = vr.gae(reward[K - 1:], values[K - 1:], boot[K - 1:], done[K - 1:], gamma, lam)
        assert not np.array_equal(wadv[0], wadv[K - 1]) and np.array_equal(wadv[K - 1], one[0])


def test_any_nonzero_done_byte_counts_as_done():
    K, E, N = 17, 9, 31
    reward, values, boot = inputs(K, E, N)
    done = done_pattern("random", K, E)
    want = vr.gae(reward, values, boot, done, 0.99, 0.95)
    odd = done.copy()
    odd[done != 0] = np.random.default_rng(3).choice(np.array([2, 0x80, 0xFF, 0x10], np.uint8), int((done != 0).sum()))
    assert odd.max() > 1 and ((odd != 0) == (done != 0)).all()
    adv, ret = run_kernel(reward, values, boot, odd, 0.99, 0.95)
    assert_bits(adv, want[0], "adv")
    assert_bits(ret, want[1], "ret")


def test_nan_and_inf_inputs():
    K, E, N = 9, 3, 7
    reward, values, boot = (a.copy() for a in inputs(17, 9, 31))
    reward, values, boot = reward[:K, :E, :N].copy(), values[:K, :E, :N].copy(), boot[:K, :E, :N].copy()
    reward[4, 0, 0] = np.nan
    values[5, 1, 1] = np.inf
    boot[6, 2, 2] = -np.inf
    reward[2, 0, 3], boot[2, 0, 3] = np.inf, -np.inf  # inf - inf
    values[3, 1, 4] = 2.0 ** -149
    done = done_pattern("random", K, E)
    adv, ret = run_kernel(reward, values, boot, done, 0.99, 0.95)
    wadv, wret = vr.gae(reward, values, boot, done, 0.99, 0.95)
    assert_bits(adv, wadv, "adv")
    assert_bits(ret, wret, "ret")
    assert np.isnan(wadv).any() and np.isinf(wadv).any() and np.isfinite(wadv).sum() > wadv.size // 2


def test_the_python_layer_and_empty_sizes():
    K, E, N = 17, 9, 31
    reward, values, boot = inputs(K, E, N)
    done = done_pattern("random", K, E)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    vals = torch.empty((K + 1, E, N), dtype=torch.float32, device=DEV)  # values: the first K rows of the launch's buffer
    vals[:K] = t(values)
    adv, ret = gae(t(reward), vals[:K], t(boot), t(done), 0.99, 0.95)
    wadv, wret = vr.gae(reward, values, boot, done, 0.99, 0.95)
    assert_bits(adv.cpu().numpy(), wadv, "adv")
    assert_bits(ret.cpu().numpy(), wret, "ret")
    a2, r2 = torch.empty_like(adv), torch.empty_like(ret)
    got = gae(t(reward), vals[:K], t(boot), t(done), 0.99, 0.95, adv=a2, ret=r2)
    assert got[0] is a2 and got[1] is r2 and torch.equal(a2.view(torch.int32), adv.view(torch.int32))
    # n_steps = 0 and E N = 0 do nothing: the outputs keep their prefill
    g = Guarded((4,), torch.float32, DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    L = _abi.lib()
    for K0, E0, N0 in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert L.macm_gae(p(g.t), p(g.t), p(g.t), p(g.t), K0, E0, N0, 0.99, 0.95, p(g.t), p(g.t), None) == 0
    torch.cuda.synchronize()
    assert bool((g.raw == FILL).all())
