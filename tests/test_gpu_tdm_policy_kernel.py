"""macm_policy_tdm (csrc/tdm_policy.hip, tdm_policy.hpp) against tests/tdm_policy_ref.py: logits and
actions bit for bit, hidden 16 and 32, float32 and float64 obs, with and without noise, the agents mask
NULL, all ones and mixed (skipped rows keep their prefill), agent counts 2, 3, 33, 64, 65 (and 257 at
H = 16) with row counts that are no multiple of the block, random masks with all-masked rows, obs values
with +-0, denormals, inf and NaN. Every buffer the kernel writes sits between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tdm_policy_ref as ref
from guard_bands import FILL, Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm.tdm_policy import TdmSetPolicy  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
# (N, E): E * N rows, more than one block of 256 and no multiple of it
SHAPES = [(2, 129), (3, 87), (33, 9), (64, 5), (65, 5)]


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def inputs(N, E):
    """(obs float64 [E, N, N-1, 4], mask, health): random slots over several magnitudes (not float32 values,
    so a float64 world's rounding is part of the test) with crafted values sprinkled over live and masked
    slots alike, random masks, and rows with no live slot and with every slot live."""
    rng = np.random.default_rng(1000 + N)
    S = N - 1
    obs = rng.standard_normal((E, N, S, 4)) * 10.0 ** rng.integers(-3, 2, (E, N, S, 1))
    d = 2.0 ** -149
    crafted = np.array([0.0, -0.0, d, -d, 1000 * d, 2.0 ** -126 * (1 - 2.0 ** -30), np.inf, -np.inf, np.nan,
                        1 + 2.0 ** -24, 2.0 ** 20])
    hit = rng.random(obs.shape) < 0.03
    obs[hit] = rng.choice(crafted, int(hit.sum()))
    mask = (rng.random((E, N, S)) < 0.6).astype(np.uint8)
    flat = mask.reshape(E * N, S)
    flat[::7] = 0  # no live slot: a dead agent, or the last one standing
    flat[3::11] = 1
    health = rng.random((E, N)) * 1.5 - 0.5
    health.reshape(-1)[::5] = 0.0
    return obs, mask, health


@functools.lru_cache(maxsize=None)
def noise_for(N, E):
    n = ref.gumbel_noise((E, N, ref.N_LOGITS), 17)
    n.reshape(-1, ref.N_LOGITS)[3 % (E * N), 1] = np.nan  # NaN noise: that z is never chosen
    n.reshape(-1, ref.N_LOGITS)[5 % (E * N), :] = np.inf
    return n


@functools.lru_cache(maxsize=None)
def reference(N, E, H, f64):
    """(logits, actions without noise, actions with noise) of the seeded weights over inputs(N, E)"""
    obs, mask, health = inputs(N, E)
    obs = obs if f64 else obs.astype(F32)
    lg = ref.logits_of(ref.seeded_params(H), H, obs, mask, health)
    return lg, ref.actions_of(lg), ref.actions_of(lg, noise_for(N, E))


def make_policy(H, params=None):
    pol = TdmSetPolicy(H, DEV)
    pol.params.copy_(torch.from_numpy(ref.seeded_params(H) if params is None else params))
    return pol


def run_kernel(pol, obs, mask, health, noise, want_logits, agents=None):
    """macm_policy_tdm through the C-ABI into guarded buffers; (actions, logits or None) as Guarded"""
    E, N = health.shape
    rows = E * N
    o = torch.from_numpy(np.ascontiguousarray(obs)).to(DEV)
    m = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    h = torch.from_numpy(np.ascontiguousarray(health)).to(DEV)
    act = Guarded((rows, 4), torch.uint8, DEV)
    lg = Guarded((rows, ref.N_LOGITS), torch.float32, DEV) if want_logits else None
    nz = torch.from_numpy(np.ascontiguousarray(noise)).to(DEV) if noise is not None else None
    ag = torch.from_numpy(np.ascontiguousarray(agents, np.uint8)).to(DEV) if agents is not None else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _abi.check(_abi.lib().macm_policy_tdm(ctypes.byref(pol.struct()), p(o), p(m), p(h), 1 if obs.dtype == np.float64 else 0,
                                          N, rows, p(ag), p(nz), p(act.t), p(lg.t) if lg else None, None),
               "macm_policy_tdm")
    torch.cuda.synchronize()
    assert act.bands_intact(), "a store outside the actions buffer"
    assert lg is None or lg.bands_intact(), "a store outside the logits buffer"
    return act, lg


def assert_bits(got, want, what):
    bad = np.argwhere(~ref.same_bits(got, want))  # bit for bit; a NaN's sign and payload are left open
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} logits differ, first at {bad[0]}: " \
                          f"got {bits(got)[tuple(bad[0])]:#x} want {bits(want)[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("with_noise", [False, True], ids=["argmax", "noise"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [16, 32])
@pytest.mark.parametrize("N,E", SHAPES)
def test_random_and_crafted_rows(N, E, H, f64, with_noise):
    obs, mask, health = inputs(N, E)
    obs = obs if f64 else obs.astype(F32)
    assert (E * N) % 256 != 0 and E * N > 256
    lg_ref, a_plain, a_noise = reference(N, E, H, f64)
    act, lg = run_kernel(make_policy(H), obs, mask, health, noise_for(N, E) if with_noise else None, True)
    assert_bits(lg.t.cpu().numpy(), lg_ref.reshape(-1, ref.N_LOGITS), f"N {N} H {H}")
    want = (a_noise if with_noise else a_plain).reshape(-1, 4)
    bad = np.argwhere(act.t.cpu().numpy() != want)
    assert bad.size == 0, f"{len(bad)} actions differ, first at {bad[0]}"
    if with_noise:
        assert set(np.unique(want[:, :3])) == {0, 1, 2} and set(np.unique(want[:, 3])) == {0, 1}, "the decisions differ"
    assert (mask.reshape(E * N, -1).sum(1) == 0).any(), "a row without a live slot is among the rows"


def test_257_agents_one_env():
    N, E, H = 257, 1, 16
    obs, mask, health = inputs(N, E)
    lg_ref, a_plain, _ = reference(N, E, H, True)
    act, lg = run_kernel(make_policy(H), obs, mask, health, None, True)
    assert_bits(lg.t.cpu().numpy(), lg_ref.reshape(-1, ref.N_LOGITS), "N 257")
    assert np.array_equal(act.t.cpu().numpy(), a_plain.reshape(-1, 4))


def test_no_logits_wanted():
    N, E, H = 33, 9, 32
    obs, mask, health = inputs(N, E)
    _, _, a_noise = reference(N, E, H, True)
    act, lg = run_kernel(make_policy(H), obs, mask, health, noise_for(N, E), False)
    assert lg is None and np.array_equal(act.t.cpu().numpy(), a_noise.reshape(-1, 4))


@pytest.mark.parametrize("kind", ["null", "ones", "mixed"])
@pytest.mark.parametrize("N,E", [(3, 87), (33, 9), (65, 5)])
def test_agents_mask(N, E, kind):
    H = 32
    obs, mask, health = inputs(N, E)
    lg_ref, a_plain, _ = reference(N, E, H, True)
    agents = {"null": None, "ones": np.ones(N, np.uint8), "mixed": (np.arange(N) % 3 != 1).astype(np.uint8)}[kind]
    act, lg = run_kernel(make_policy(H), obs, mask, health, None, True, agents)
    taken = np.tile(np.ones(N, bool) if agents is None else agents.astype(bool), E)
    assert act.rows_untouched(~taken) and lg.rows_untouched(~taken), "a skipped row was written"
    assert_bits(lg.t.cpu().numpy()[taken], lg_ref.reshape(-1, ref.N_LOGITS)[taken], kind)
    assert np.array_equal(act.t.cpu().numpy()[taken], a_plain.reshape(-1, 4)[taken])
    if kind == "mixed":
        assert taken.any() and not taken.all()
        assert (act.t.cpu().numpy()[~taken] == FILL).all()


def test_python_layer_and_linear_layers():
    """TdmSetPolicy.act over [E, N, ...] tensors, the bot's actions first and the policy's over them; params
    from nn.Linear layers, transposed to [in][out]."""
    N, E, H = 33, 9, 16
    obs, mask, health = inputs(N, E)
    lg_ref, a_plain, a_noise = reference(N, E, H, False)
    params = ref.seeded_params(H)
    ws, bs = ref.split_params(params, H)
    layers = [torch.nn.Linear(i, o) for i, o in ref.layer_shapes(H)]
    with torch.no_grad():
        for lin, w, b in zip(layers, ws, bs):
            lin.weight.copy_(torch.from_numpy(w.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
    pol = TdmSetPolicy.from_linear_layers(layers, device=DEV)
    assert np.array_equal(pol.params.cpu().numpy(), params) and pol.params.numel() == ref.n_params(H)
    o = torch.from_numpy(obs.astype(F32)).to(DEV)
    m, h = torch.from_numpy(mask).to(DEV), torch.from_numpy(health).to(DEV)
    lg = torch.empty((E, N, ref.N_LOGITS), dtype=torch.float32, device=DEV)
    a = pol.act(o, m, h, logits=lg)
    assert a.shape == (E, N, 4) and np.array_equal(a.cpu().numpy(), a_plain)
    assert_bits(lg.cpu().numpy(), lg_ref, "TdmSetPolicy.act")
    out = torch.full((E, N, 4), 9, dtype=torch.uint8, device=DEV)
    agents = torch.from_numpy((np.arange(N) < 16).astype(np.uint8)).to(DEV)
    pol.act(o, m, h, noise=torch.from_numpy(noise_for(N, E)).to(DEV), out=out, agents=agents)
    assert np.array_equal(out.cpu().numpy()[:, :16], a_noise[:, :16]) and bool((out[:, 16:] == 9).all())
    # torch_logits on the device: the same function within float32 rounding (no bit claim)
    # (rows with a NaN or inf in a live slot apart: torch's relu passes a NaN on, the definition's gives +0)
    fin = np.isfinite(lg_ref).all(-1) & ~(~np.isfinite(obs) & (mask[..., None] != 0)).any((-1, -2))
    tl = pol.torch_logits(o, m, h).cpu().numpy()
    assert fin.sum() > fin.size // 2 and np.allclose(tl[fin], lg_ref[fin], rtol=1e-3, atol=1e-3)
    with pytest.raises(ValueError):
        TdmSetPolicy(24, DEV)
    with pytest.raises(ValueError):
        pol.act(o, m, h, agents=agents)  # agents without out
