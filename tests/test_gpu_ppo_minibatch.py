"""macm_ppo_grad_rows and macm_adv_moments (PPO over shuffled minibatches, include/macm.h) on the device.

The contract is bits: macm_ppo_grad_rows(index) gives, in both gradients and all eight stats, what macm_ppo_grad
gives on torch-gathered contiguous copies of the inputs, for every supported shape, float32 and float64 obs,
row counts of one lane, a tile and a lane either side, many waves and past the cap on the waves, both nets and
either alone, with and without the clipped value loss, and for index patterns of every kind (identity,
reversed, a permutation's prefix, sampling with replacement, one row repeated, a block-shuffled minibatch of
gym_macm.ppo.minibatches, whose length is the minibatch's own). With adv_norm from macm_adv_moments the
reference is the same call on copies whose adv is tests/minibatch_ref.py's normalise with the mean and rstd the
device wrote. The moments agree with minibatch_ref.moments within the bound that module derives. Indices
outside [0, n_src) add nothing and are never followed.

The source arrays have 5000 rows and each is a view inside a larger allocation whose 70 rows before and after
are poison (NaN, action bytes 255): a read outside the view shows in the results where no fault would show it.
Inputs as test_gpu_ppo_fused.py's: grad_ref.float_inputs, gradients NaN on entry, guard bands round the
outputs and the workspace."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grad_ref as gr
import minibatch_ref as M
import ppo_ref as R
from guard_bands import Guarded
from test_gpu_ppo_fused import fused, ibits, p

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import policy as P  # noqa: E402
from gym_macm import ppo  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
N_SRC, PAD = 5000, 70
BIG = 131137  # past 2048 waves of 64 rows: wave 0 takes a second tile, and the last tile holds one row
SIZES = (1, 63, 64, 129, 4097, BIG)
CASES = [(od, H, nh, 65) for od, H, nh in gr.SHAPES] + [(4, 32, 2, rows) for rows in SIZES]
PER_ROW = ("obs", "actions", "old_logp", "adv", "ret", "old_values")


def padded(a):
    """a [N_SRC, ...] as a view inside an allocation with PAD poison rows either side"""
    poison = 255 if a.dtype == np.uint8 else np.nan
    full = np.full((N_SRC + 2 * PAD,) + a.shape[1:], poison, a.dtype)
    full[PAD:PAD + N_SRC] = a
    return torch.from_numpy(full).to(DEV)[PAD:PAD + N_SRC]


@functools.lru_cache(maxsize=None)
def source(od, H, nh, f64):
    """The nets and N_SRC source rows of every input, as test_gpu_ppo_fused.case() draws them; advantages N(0.3, 1)"""
    params_p, obs, _ = gr.float_inputs("policy", od, H, nh, N_SRC)
    params_v, _, _ = gr.float_inputs("critic", od, H, nh, N_SRC)
    pol, crit = P.MlpPolicy(od, H, nh, DEV), P.MlpCritic(od, H, nh, DEV)
    pol.params.copy_(torch.from_numpy(params_p))
    crit.params.copy_(torch.from_numpy(params_v))
    tobs = padded((0.2 * obs).astype(F64 if f64 else F32))
    rng = np.random.default_rng([9100, od, H, nh])
    actions = padded(rng.integers(0, 3, (N_SRC, 3)).astype(np.uint8))
    logits = torch.empty((N_SRC, 9), dtype=torch.float32, device=DEV)
    pol.act(tobs, logits=logits)
    values = crit.value(tobs)
    n = lambda t: t.cpu().numpy()
    draw = lambda s: (s * rng.standard_normal(N_SRC)).astype(F32)
    old_logp = padded(n(ppo.log_prob(logits, actions.contiguous())) + draw(0.3))
    adv = padded(F32(0.3) + draw(1.0))
    ret = padded(n(values) + draw(1.0))
    old_values = padded(n(values) + draw(0.3))
    torch.cuda.synchronize()
    return dict(pol=pol, crit=crit, obs=tobs, rows=N_SRC, f64=f64, actions=actions, old_logp=old_logp, adv=adv,
                ret=ret, old_values=old_values)


def gathered(src, index, adv=None):
    """The contiguous copies macm_ppo_grad is called on: the source rows at index, in the dict fused() takes"""
    i = index.long()
    c = dict(src, rows=int(index.numel()))
    for k in PER_ROW:
        c[k] = src[k][i].contiguous()
    if adv is not None:
        c["adv"] = adv
    return c


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def patterns(rows, seed):
    """name -> index (int32 [rows] on the device; the minibatch pattern has the minibatch's own length)"""
    rng = np.random.default_rng([9200, rows, seed])
    perm = np.concatenate([rng.permutation(N_SRC) for _ in range(-(-rows // N_SRC))])[:rows]
    n_mb = min(max(1, N_SRC // rows), -(-N_SRC // 64))  # about `rows` rows each, and no more minibatches than blocks
    mb = ppo.minibatches(N_SRC, n_mb, generator=torch.Generator().manual_seed(seed), block=64, device=DEV)
    return {"identity": i32(np.arange(rows) % N_SRC), "reversed": i32((N_SRC - 1 - np.arange(rows)) % N_SRC),
            "permutation": i32(perm), "replacement": i32(rng.integers(0, N_SRC, rows)),
            "repeated": i32(np.full(rows, 1234)), "minibatch": mb[0]}


def through_index(src, cfg, vclip, index, norm=None, pol=True, crit=True, rows=None, n_src=N_SRC):
    """One macm_ppo_grad_rows call on the source arrays into guarded buffers: (grad_policy, grad_value, stats)"""
    rows = int(index.numel()) if index is not None else rows
    gp = Guarded((src["pol"].params.numel(),), torch.float32, DEV)
    gv = Guarded((src["crit"].params.numel(),), torch.float32, DEV)
    gp.t.fill_(float("nan"))
    gv.t.fill_(float("nan"))
    stats = Guarded((8,), torch.float64, DEV)
    ws = Guarded((ppo.workspace_bytes(rows),), torch.uint8, DEV)
    torch.cuda.synchronize()
    _abi.check(_abi.lib().macm_ppo_grad_rows(
        ctypes.byref(cfg), ctypes.byref(src["pol"].struct()) if pol else None,
        ctypes.byref(src["crit"].struct()) if crit else None, p(src["obs"]), 1 if src["f64"] else 0, rows, p(index),
        n_src, p(norm), p(src["actions"]) if pol else None, p(src["old_logp"]) if pol else None,
        p(src["adv"]) if pol else None, p(src["ret"]) if crit else None,
        p(src["old_values"]) if (crit and vclip) else None, p(gp.t) if pol else None, p(gv.t) if crit else None,
        p(stats.t), p(ws.t), ws.t.numel(), None), "macm_ppo_grad_rows")
    torch.cuda.synchronize()
    for name, g in (("grad_policy", gp), ("grad_value", gv), ("stats", stats), ("workspace", ws)):
        assert g.bands_intact(), f"a store outside {name}"
    return gp.t, gv.t, stats.t


def moments(x, index, rows=None, eps=1e-8, n_src=N_SRC):
    """One macm_adv_moments call into a guarded out: the float64 [4] device tensor"""
    rows = int(index.numel()) if index is not None else rows
    out = Guarded((4,), torch.float64, DEV)
    ws = Guarded((max(ppo.workspace_bytes(rows), 16),), torch.uint8, DEV)
    torch.cuda.synchronize()
    _abi.check(_abi.lib().macm_adv_moments(p(x), p(index), n_src, rows, eps, p(out.t), p(ws.t), ws.t.numel(), None),
               "macm_adv_moments")
    torch.cuda.synchronize()
    assert out.bands_intact() and ws.bands_intact(), "a store outside out or the workspace"
    return out.t


def same(got, want, what, pol=True, crit=True, nonzero=True):
    """got's bits are want's; nonzero: the reference's gradients are not all zero (a single row, or one row
    repeated, may have a clipped value loss, whose gradient is zero)"""
    gp, gv, gs = got
    wp, wv, ws = want
    if pol:
        assert bool(torch.isfinite(gp).all()) and (float(wp.abs().max()) > 0 or not nonzero), what
        assert torch.equal(ibits(gp), ibits(wp)), f"{what}: the policy's gradient"
    else:
        assert bool(torch.isnan(gp).all()), f"{what}: grad_policy is not written"
    if crit:
        assert bool(torch.isfinite(gv).all()) and (float(wv.abs().max()) > 0 or not nonzero), what
        assert torch.equal(ibits(gv), ibits(wv)), f"{what}: the critic's gradient"
    else:
        assert bool(torch.isnan(gv).all()), f"{what}: grad_value is not written"
    assert bool(torch.isfinite(gs).all()) and torch.equal(gs.view(torch.int64), ws.view(torch.int64)), f"{what}: stats"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh,rows", CASES)
def test_bits_of_the_contiguous_call(od, H, nh, rows, f64):
    src = source(od, H, nh, f64)
    vclip = (H == 32) == (nh == 2)  # half of the shapes with the clipped value loss, and below the other half
    cfg = lambda v: ppo.config(vf_clip=R.VF_CLIP if v else None)
    pats = patterns(rows, int(f64))
    for name, index in pats.items():
        assert name == "minibatch" or index.numel() == rows
        want = fused(gathered(src, index), cfg(vclip), vclip)
        same(through_index(src, cfg(vclip), vclip, index), want, f"{name} {index.numel()}", nonzero=name != "repeated" and rows > 1)
    index = pats["permutation"]
    for pol, crit, v in ((True, False, vclip), (False, True, vclip), (False, True, not vclip), (True, True, not vclip)):
        want = fused(gathered(src, index), cfg(v), v, pol=pol, crit=crit)
        same(through_index(src, cfg(v), v, index, pol=pol, crit=crit), want, f"pol {pol} crit {crit} vclip {v}", pol, crit, nonzero=rows > 1)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_identity_over_the_whole_array_is_the_contiguous_call(f64):
    src = source(4, 32, 2, f64)
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    same(through_index(src, cfg, True, i32(np.arange(N_SRC))), fused(src, cfg, True), "identity")


@pytest.mark.parametrize("od,H,nh,rows", [(4, 32, 2, 4097), (6, 16, 1, 65), (4, 32, 2, BIG)])
def test_normalised_advantages(od, H, nh, rows):
    src = source(od, H, nh, False)
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    index = patterns(rows, 2)["permutation"]
    for idx in (index, None):  # through the index, and with positions as rows over the whole array
        n = rows if idx is not None else N_SRC
        out = moments(src["adv"], idx, rows=n)
        mean, rstd = out.cpu().numpy()[:2]  # the bits the device wrote
        c = gathered(src, idx if idx is not None else i32(np.arange(N_SRC)))
        c["adv"] = torch.from_numpy(M.normalise(c["adv"].cpu().numpy(), mean, rstd)).to(DEV)
        assert abs(float(c["adv"].mean())) < 1e-3 and abs(float(c["adv"].std()) - 1) < 1e-3
        got = through_index(src, cfg, True, idx, norm=out, rows=n)
        same(got, fused(c, cfg, True), f"normalised, index {'given' if idx is not None else 'NULL'}")
        raw = through_index(src, cfg, True, idx, rows=n) if idx is not None else fused(src, cfg, True)
        assert not torch.equal(ibits(raw[0]), ibits(got[0])), "the normalisation changes the policy's gradient"
        assert torch.equal(ibits(raw[1]), ibits(got[1])), "and leaves the critic's alone"


@pytest.mark.parametrize("rows", (1, 2) + SIZES[1:] + (65,))
def test_moments_within_the_derived_bound(rows):
    src = source(4, 32, 2, False)
    x = src["adv"]
    xs = x.cpu().numpy()
    rng = np.random.default_rng([9300, rows])
    cases = {"replacement": i32(rng.integers(0, N_SRC, rows))}
    if rows <= N_SRC:
        cases["NULL"] = None
    for name, index in cases.items():
        out = moments(x, index, rows=rows)
        again = moments(x, index, rows=rows)
        assert torch.equal(out.view(torch.int64), again.view(torch.int64)), "two calls, the same bits"
        got = out.cpu().numpy()
        ref = M.moments(xs[:rows] if index is None else xs, None if index is None else index.cpu().numpy(), 1e-8)
        bound = M.bounds(ref)
        assert got[3] == rows == ref["n"]
        if rows == 1:
            assert got[2] == 0.0 and got[1] == 1.0 / 1e-8 and got[0] == ref["mean"]
        for g, name_ in ((got[0], "mean"), (got[1], "rstd"), (got[2], "std")):
            err = abs(g - ref[name_])
            share = err / bound[name_] if bound[name_] > 0 else 0.0
            print(f"moments rows {rows} index {name}: {name_} {g!r} err {err:.3e} bound {bound[name_]:.3e} share {share:.4f}")
            assert err <= bound[name_], (name_, g, ref[name_], bound[name_])


def test_zero_rows_and_eps():
    src = source(4, 32, 2, False)
    got = moments(src["adv"], None, rows=0, eps=1e-5).cpu().numpy()
    assert got.tolist() == [0.0, 1.0 / 1e-5, 0.0, 0.0]
    got = moments(src["adv"], i32(np.arange(100)), eps=0.5).cpu().numpy()
    ref = M.moments(src["adv"].cpu().numpy(), np.arange(100), 0.5)
    assert abs(got[1] - ref["rstd"]) <= M.bounds(ref)["rstd"] and got[3] == 100


def test_bad_indices_add_nothing_and_are_never_followed():
    src = source(4, 32, 2, False)
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    valid = patterns(64, 4)["permutation"]
    outside = [-1, -PAD, N_SRC, N_SRC + PAD - 1, -2, N_SRC + 1, -PAD // 2, N_SRC + PAD // 2]  # inside the poison rows
    bad = torch.cat([valid, i32(np.resize(outside, 64))])
    assert bad.numel() == 128 and bool(torch.isnan(src["adv"].as_strided((1,), (1,), src["adv"].storage_offset() - 1)).all())
    gp, gv, stats = through_index(src, cfg, True, bad)
    hp, hv, hstats = through_index(src, cfg, True, valid)
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all()) and bool(torch.isfinite(stats).all())
    tiny = 2.0 ** -125  # half of it is still a normal float32
    for h in (hp, hv):
        assert bool(((h.abs() >= tiny) | (h == 0)).all()), "none of this seed's gradient elements is subnormal"
    # 1/128 and 1/64 are powers of two and the second tile adds exact zeros
    assert torch.equal(ibits(gp), ibits(0.5 * hp)) and torch.equal(ibits(gv), ibits(0.5 * hv))
    s, h = stats.cpu().numpy(), hstats.cpu().numpy()
    assert s[7] == 128.0 and h[7] == 64.0
    assert s[6] == h[6] and np.array_equal(s[:6], 0.5 * h[:6]), "the sums are the valid positions', over rows = 128"
    out, alone = moments(src["adv"], bad).cpu().numpy(), moments(src["adv"], valid).cpu().numpy()
    assert out[3] == 64.0 and np.array_equal(out.view(np.int64), alone.view(np.int64))
    # with the normalisation too, and with n_src = 0 every position is outside
    norm = moments(src["adv"], bad)
    np_, _, nstats = through_index(src, cfg, True, bad, norm=norm)
    vp, _, _ = through_index(src, cfg, True, valid, norm=norm)
    assert bool(torch.isfinite(nstats).all()) and torch.equal(ibits(np_), ibits(0.5 * vp))
    zp, zv, zs = through_index(src, cfg, True, valid, n_src=0)
    assert not zp.any() and not zv.any() and zs.cpu().numpy().tolist() == [0.0] * 7 + [64.0]


def test_ppo_grads_with_index_and_adv_norm():
    src = dict(source.__wrapped__(4, 32, 2, False))  # nets of its own: it sets requires_grad and .grad on them
    pol, crit = src["pol"], src["crit"]
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    index = patterns(4097, 5)["permutation"]
    args = (src["obs"], src["actions"], src["old_logp"], src["adv"], src["ret"])
    kw = dict(old_values=src["old_values"], vf_clip=R.VF_CLIP)
    norm = ppo.adv_moments(src["adv"], index)
    assert torch.equal(norm.view(torch.int64), moments(src["adv"], index).view(torch.int64))
    gp, gv, stats = through_index(src, cfg, True, index, norm=norm)
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    pol.params.grad = crit.params.grad = None
    s1 = ppo.ppo_grads(pol, crit, *args, index=index, adv_norm=norm, **kw)
    assert torch.equal(ibits(pol.params.grad), ibits(gp)) and torch.equal(ibits(crit.params.grad), ibits(gv))
    assert torch.equal(s1.view(torch.int64), stats.view(torch.int64))
    s2 = ppo.ppo_grads(pol, crit, *args, index=index.long(), adv_norm=norm[:2].clone(), **kw)  # int64: converted
    assert torch.equal(ibits(pol.params.grad), ibits(gp + gp)) and torch.equal(ibits(crit.params.grad), ibits(gv + gv))
    assert torch.equal(s2.view(torch.int64), stats.view(torch.int64))
    # leading dimensions are flattened into n_src source rows
    pol.params.grad = crit.params.grad = None
    shaped = [t.view((50, 100) + t.shape[1:]) for t in args]
    ppo.ppo_grads(pol, crit, *shaped, index=index, adv_norm=norm, old_values=src["old_values"].view(50, 100), vf_clip=R.VF_CLIP)
    assert torch.equal(ibits(pol.params.grad), ibits(gp)) and torch.equal(ibits(crit.params.grad), ibits(gv))
    # adv_norm alone: positions are rows
    pol.params.grad = crit.params.grad = None
    whole = ppo.adv_moments(src["adv"])
    ppo.ppo_grads(pol, crit, *args, adv_norm=whole, **kw)
    wp, wv, _ = through_index(src, cfg, True, None, norm=whole, rows=N_SRC)
    assert torch.equal(ibits(pol.params.grad), ibits(wp)) and torch.equal(ibits(crit.params.grad), ibits(wv))
    # one epoch touches every row once: the rows and the clipped rows of the four calls add up to the array's
    full = ppo.ppo_grads(pol, crit, *args, **kw).cpu().numpy()
    mbs = ppo.minibatches(N_SRC, 4, generator=torch.Generator().manual_seed(6), device=DEV)
    per = [ppo.ppo_grads(pol, crit, *args, index=mb, **kw).cpu().numpy() for mb in mbs]
    assert sum(s[7] for s in per) == N_SRC == full[7]
    clipped = [s[5] * s[7] for s in per]
    assert all(abs(c - round(c)) < 1e-6 for c in clipped) and round(full[5] * N_SRC) > 0
    assert sum(round(c) for c in clipped) == round(full[5] * N_SRC)
    assert max(s[6] for s in per) == full[6]
