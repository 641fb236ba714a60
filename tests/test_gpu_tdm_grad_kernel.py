"""macm_tdm_policy_grad (csrc/tdm_policy_grad.hip) through the C-ABI against tests/tdm_grad_ref.py: both hidden
sizes with float32 and float64 obs at agent counts from 2 to 65; integer inputs, on which every association of
the sums gives the same float32 and the device must equal the reference exactly (ties between slots included), at
row counts around a tile, over several waves and past the cap on the partials; float inputs within
tdm_grad_ref.tol; the constructed rows of tests/test_tdm_grad_ref.py. In every call obs, health and dlogits carry
NaN rows after `rows` under a mask of ones (a tail lane that read them would show as NaN), grad starts as NaN (it
is overwritten, not accumulated), and grad and the workspace sit between guard bands."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tdm_grad_ref as tg
from guard_bands import Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import policy as P  # noqa: E402
from gym_macm import tdm_policy as TP  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
TAIL = 70  # NaN rows behind the rows of a call: more than a tile
AGENTS = (2, 3, 9, 33, 65)
# past the cap, at N = 2: tiles 0, cap and 2 cap belong to wave 0, and the last tile (2 cap + 1) holds two rows
BIG = 2 * P.GRAD_TILE_ROWS * P.GRAD_MAX_PARTIALS + P.GRAD_TILE_ROWS + 2


def envs_near(n_agents, target):
    return max(1, round(target / n_agents))


def row_cases(targets, big):
    """(n_agents, envs): rows = n_agents * envs nearest to each target, once each; the BIG count at N = 2."""
    out = []
    for n in AGENTS:
        for e in sorted({envs_near(n, t) for t in targets}):
            out.append((n, e))
    if big:
        out.append((2, BIG // 2))
    return out


INT_CASES = row_cases((63, 64, 65, 257), big=True)  # a tile - 1, a tile, a tile + 1, a few tiles
FLOAT_CASES = row_cases((65, 1000), big=False)


def workspace_bytes(rows):
    n = ctypes.c_int64(-1)
    _abi.check(_abi.lib().macm_tdm_grad_workspace(rows, ctypes.byref(n)), "macm_tdm_grad_workspace")
    return n.value


def make_policy(H, params):
    m = TP.TdmSetPolicy(H, DEV)
    m.params.copy_(torch.from_numpy(np.ascontiguousarray(params, F32)))
    return m


def with_tail(a, dtype, fill):
    """[rows, ...] on the device with TAIL rows of `fill` behind"""
    full = np.full((a.shape[0] + TAIL,) + a.shape[1:], fill, dtype)
    full[:a.shape[0]] = a
    return torch.from_numpy(full).to(DEV)


def run_grad(m, c, f64, n_agents, rows=None, agents=None, stream=None):
    """One call through the C-ABI into guarded buffers; the gradient as numpy. c: obs [E, N, N-1, 4] (or flat
    rows), mask, health, dlogits."""
    S = n_agents - 1
    n = c["mask"].reshape(-1, S).shape[0]
    rows = n if rows is None else rows
    tobs = with_tail(c["obs"].reshape(n, S, 4), F64 if f64 else F32, np.nan)
    tmask = with_tail(c["mask"].reshape(n, S), np.uint8, 1)
    thealth = with_tail(c["health"].reshape(n), F64, np.nan)
    tdl = with_tail(c["dlogits"].reshape(n, tg.N_LOGITS), F32, np.nan)
    tag = torch.from_numpy(np.ascontiguousarray(agents, np.uint8)).to(DEV) if agents is not None else None
    grad = Guarded((m.params.numel(),), torch.float32, DEV)
    grad.t.fill_(float("nan"))
    nbytes = workspace_bytes(rows)
    ws = Guarded((max(nbytes, 16),), torch.uint8, DEV)
    torch.cuda.synchronize()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _abi.check(_abi.lib().macm_tdm_policy_grad(
        ctypes.byref(m.struct()), vp(tobs), vp(tmask), vp(thealth), 1 if f64 else 0, n_agents, rows, vp(tag), vp(tdl),
        vp(grad.t), vp(ws.t) if nbytes else None, nbytes,
        ctypes.c_void_p(stream.cuda_stream) if stream is not None else None), "macm_tdm_policy_grad")
    torch.cuda.synchronize()
    assert grad.bands_intact(), "a store outside grad"
    assert ws.bands_intact(), "a store outside the workspace"
    return grad.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def integer_case(H, n_agents, envs):
    c = tg.integer_inputs(H, n_agents, envs)
    g, G = tg.case_grad(c, H)
    fwd = tg.forward(c["params"], H, c["obs"], c["mask"], c["health"])
    return c, g, G, tg.tied_units(fwd)


@functools.lru_cache(maxsize=None)
def float_case(H, n_agents, envs):
    c = tg.float_inputs(H, n_agents, envs)
    return c, tg.case_grad(c, H)


def assert_equal(got, want, ctx):
    bad = np.argwhere(got != want)  # (a NaN differs from everything; the sign of a zero sum is left open)
    assert bad.size == 0, f"{ctx}: {len(bad)} of {want.size} differ, first at {bad[0][0]}: got {got[bad[0][0]]} " \
                          f"want {want[bad[0][0]]}"


@pytest.mark.parametrize("n_agents,envs", INT_CASES)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [16, 32])
def test_integer_inputs_equal_the_reference(H, f64, n_agents, envs):
    c, g, G, tied = integer_case(H, n_agents, envs)
    rows = n_agents * envs
    assert G.max() < 2 ** 24, "every partial sum is an exact float32 integer"
    assert (c["mask"].reshape(rows, -1).sum(axis=1) == 0).any(), "an empty set among the rows"
    assert (c["mask"].reshape(rows, -1).sum(axis=1) < n_agents - 1).any() or n_agents == 2, "dead agents"
    if n_agents > 2:  # (one slot cannot tie)
        assert tied > 0, "ties between slots of different content"
    got = run_grad(make_policy(H, c["params"]), c, f64, n_agents)
    want = g.astype(F32)
    assert_equal(got, want, f"H {H} N {n_agents} rows {rows}")
    sl = tg.layer_slices(H)
    assert np.count_nonzero(want) > want.size // 8, "the gradient is not trivially zero"
    assert np.count_nonzero(want[sl["W1"]]) > 0 and np.count_nonzero(want[sl["b1"]]) > 0, "nor is layer 1's"


@pytest.mark.parametrize("n_agents,envs", FLOAT_CASES)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [16, 32])
def test_float_inputs_within_the_bound(H, f64, n_agents, envs):
    c, (g, G) = float_case(H, n_agents, envs)
    rows = n_agents * envs
    if not f64:  # the float32 call's slots are other numbers than the float64 call's: a reference of its own
        c = dict(c, obs=c["obs"].astype(F32))
        g, G = tg.case_grad(c, H)
    got = run_grad(make_policy(H, c["params"]), c, f64, n_agents).astype(F64)
    bound = tg.tol(G, rows, H)
    used = np.abs(got - g)[G > 0] / bound[G > 0]
    print(f"H {H} N {n_agents} rows {rows} {'f64' if f64 else 'f32'}: {used.max():.4f} of the bound")
    assert np.isfinite(got).all()
    assert used.max() <= 1.0, used.max()
    assert not got[G == 0].any()


@pytest.mark.parametrize("name", tg.CONSTRUCTED)
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [16, 32])
def test_constructed_rows(H, f64, name):
    """The rows of tests/test_tdm_grad_ref.py (small integers and halves: exact in any association): the lowest
    tied slot, a masked slot of inf and NaN, the empty set, units whose every e is <= 0, skipped NaN rows."""
    c = tg.constructed_case(name, H)
    g, _ = tg.case_grad(c, H)
    got = run_grad(make_policy(H, c["params"]), c, f64, 3, agents=c["agents"])
    assert np.isfinite(got).all()
    assert_equal(got, g.astype(F32), name)
    sl = tg.layer_slices(H)
    if name == "tie":
        assert got[sl["W1"]].reshape(4, H)[2, 0] == 5, "the lowest tied slot took the gradient"
    if name in ("empty", "nonpos"):
        assert not got[sl["W1"]].any() and not got[sl["b1"]].any()
        assert got[sl["b2"]][2] == 3


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("H", [16, 32])
def test_agents_skip_rows(H, f64):
    """agents given: the skipped rows hold NaN (obs, health, dlogits) under a mask of ones. A call on the kept
    rows alone puts them at other lanes and tiles, so its sums associate differently: the two agree exactly on
    integer inputs and within the bound on float inputs."""
    N, E = 5, 30  # 150 rows, 90 kept: both calls span more than one tile
    agents = np.array([1, 0, 1, 1, 0], np.uint8)
    keep = agents.astype(bool)
    for kind, make in (("int", tg.integer_inputs), ("float", tg.float_inputs)):
        c = make(H, N, E)
        if not f64:
            c = dict(c, obs=c["obs"].astype(F32))
        g, G = tg.case_grad(dict(c, agents=agents), H)
        dirty = {k: np.array(c[k], copy=True) for k in ("obs", "mask", "health", "dlogits")}
        for k in ("obs", "health", "dlogits"):
            dirty[k][:, ~keep] = np.nan
        dirty["mask"][:, ~keep] = 1
        m = make_policy(H, c["params"])
        got = run_grad(m, dirty, f64, N, agents=agents)
        alone = run_grad(m, {k: np.ascontiguousarray(c[k][:, keep]) for k in dirty}, f64, N)
        assert np.isfinite(got).all() and np.isfinite(alone).all()
        if kind == "int":
            assert G.max() < 2 ** 24
            assert_equal(got, g.astype(F32), "agents")
            assert_equal(alone, got, "the kept rows alone")
            assert np.count_nonzero(got) > got.size // 8
        else:
            bound = tg.tol(G, N * E, H)
            for x in (got, alone):
                assert (np.abs(x.astype(F64) - g) <= bound).all()


def test_same_arguments_same_bits_on_any_stream():
    H, N, E = 32, 9, 7112  # 64,008 rows, 1001 tiles: many waves in flight, none with the same timing twice
    c = tg.float_inputs(H, N, E)
    c = dict(c, obs=c["obs"].astype(F32))
    m = make_policy(H, c["params"])
    a = run_grad(m, c, False, N)
    b = run_grad(m, c, False, N)
    s = run_grad(m, c, False, N, stream=torch.cuda.Stream(DEV))
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("H", [16, 32])
def test_zero_rows_writes_zeros(H):
    c = tg.float_inputs(H, 3, 2)
    got = run_grad(make_policy(H, c["params"]), c, True, 3, rows=0)  # no workspace: NULL, 0 bytes
    assert got.shape == (tg.n_params(H),)
    assert np.array_equal(got.view(np.uint32), np.zeros(got.shape, np.uint32))
