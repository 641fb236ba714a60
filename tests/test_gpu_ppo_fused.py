"""macm_ppo_grad (the PPO loss inside the gradient launches, csrc/policy_grad.hip) against the chain it fuses:
macm_policy_flock's logits (macm_value_flock's values) -> macm_ppo_loss -> macm_policy_grad (macm_value_grad)
on the same inputs, bit for bit, for every supported shape of both nets, float32 and float64 obs, row counts
of one lane, a tile and a lane, many waves, and past the cap on the waves; its stats against tests/ppo_ref.py
on the chain's logits and values within ppo_ref's bound; either net left out; gym_macm.ppo.ppo_grads
accumulating into an existing .grad; and two calls giving the same bits. obs carries NaN rows after `rows`,
the gradients start as NaN and sit between guard bands with the workspace."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grad_ref as gr
import ppo_ref as R
from guard_bands import FILL, Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import policy as P  # noqa: E402
from gym_macm import ppo  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
TAIL = 70
BIG = 131137  # past 2048 waves of 64 rows: wave 0 takes a second tile, and the last tile holds one row
CASES = [(od, H, nh, rows) for od, H, nh in gr.SHAPES for rows in (1, 65, 4097)] + [(4, 32, 2, BIG)]


def ibits(t):
    return t.detach().contiguous().view(torch.int32)


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@functools.lru_cache(maxsize=None)
def case(od, H, nh, rows, f64):
    """The nets, the obs rows (with a NaN tail) and the loss's inputs; old_logp around the nets' own logp"""
    params_p, obs, _ = gr.float_inputs("policy", od, H, nh, rows)
    params_v, _, _ = gr.float_inputs("critic", od, H, nh, rows)
    pol, crit = P.MlpPolicy(od, H, nh, DEV), P.MlpCritic(od, H, nh, DEV)
    pol.params.copy_(torch.from_numpy(params_p))
    crit.params.copy_(torch.from_numpy(params_v))
    full = np.full((rows + TAIL, od), np.nan, F64 if f64 else F32)
    full[:rows] = 0.2 * obs  # (logits of a few units: ratios and probabilities of every size)
    tobs = torch.from_numpy(full).to(DEV)[:rows]
    rng = np.random.default_rng([9000, od, H, nh, rows])
    actions = torch.from_numpy(rng.integers(0, 3, (rows, 3)).astype(np.uint8)).to(DEV)
    logits = torch.empty((rows, 9), dtype=torch.float32, device=DEV)
    pol.act(tobs, logits=logits)
    values = crit.value(tobs)
    f = lambda a: torch.from_numpy(a.astype(F32)).to(DEV)
    old_logp = ppo.log_prob(logits, actions) + f(0.3 * rng.standard_normal(rows))
    adv, ret = f(rng.standard_normal(rows)), values + f(rng.standard_normal(rows))
    old_values = values + f(0.3 * rng.standard_normal(rows))
    return dict(pol=pol, crit=crit, obs=tobs, rows=rows, f64=f64, actions=actions, logits=logits, values=values,
                old_logp=old_logp.contiguous(), adv=adv, ret=ret.contiguous(), old_values=old_values.contiguous())


def fused(c, cfg, vclip, pol=True, crit=True, stream=None, want_stats=True):
    """One macm_ppo_grad call into guarded buffers: (grad_policy, grad_value, stats) as device tensors; without
    want_stats the stats pointer is NULL and the buffer must keep its fill"""
    rows = c["rows"]
    gp, gv = Guarded((c["pol"].params.numel(),), torch.float32, DEV), Guarded((c["crit"].params.numel(),), torch.float32, DEV)
    gp.t.fill_(float("nan"))
    gv.t.fill_(float("nan"))
    stats = Guarded((8,), torch.float64, DEV)
    ws = Guarded((ppo.workspace_bytes(rows),), torch.uint8, DEV)
    torch.cuda.synchronize()
    _abi.check(_abi.lib().macm_ppo_grad(
        ctypes.byref(cfg), ctypes.byref(c["pol"].struct()) if pol else None,
        ctypes.byref(c["crit"].struct()) if crit else None, p(c["obs"]), 1 if c["f64"] else 0, rows,
        p(c["actions"]) if pol else None, p(c["old_logp"]) if pol else None, p(c["adv"]) if pol else None,
        p(c["ret"]) if crit else None, p(c["old_values"]) if (crit and vclip) else None, p(gp.t) if pol else None,
        p(gv.t) if crit else None, p(stats.t) if want_stats else None, p(ws.t), ws.t.numel(),
        ctypes.c_void_p(stream.cuda_stream) if stream is not None else None), "macm_ppo_grad")
    torch.cuda.synchronize()
    for name, g in (("grad_policy", gp), ("grad_value", gv), ("stats", stats), ("workspace", ws)):
        assert g.bands_intact(), f"a store outside {name}"
    assert want_stats or bool((stats.bytes == FILL).all()), "stats was not wanted and was written"
    return gp.t, gv.t, stats.t


def chain(c, cfg, vclip):
    """logits / values -> macm_ppo_loss -> macm_policy_grad / macm_value_grad: (grad_policy, grad_value)"""
    rows = c["rows"]
    ws = torch.empty((ppo.workspace_bytes(rows),), dtype=torch.uint8, device=DEV)
    dl, dv = torch.empty_like(c["logits"]), torch.empty_like(c["values"])
    _abi.check(_abi.lib().macm_ppo_loss(ctypes.byref(cfg), rows, p(c["logits"]), p(c["actions"]), p(c["old_logp"]),
                                        p(c["adv"]), p(c["values"]), p(c["ret"]), p(c["old_values"]) if vclip else None,
                                        None, p(dl), p(dv), None, p(ws), ws.numel(), None), "macm_ppo_loss")
    torch.cuda.synchronize()
    return c["pol"].param_grad(c["obs"], dl), c["crit"].param_grad(c["obs"], dv)


def reference(c, vclip, **kw):
    n = lambda t: t.cpu().numpy()
    return R.loss(n(c["logits"]), n(c["actions"]), n(c["old_logp"]), n(c["adv"]), n(c["values"]), n(c["ret"]),
                  n(c["old_values"]) if vclip else None, vf_clip=R.VF_CLIP if vclip else None, **kw)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("od,H,nh,rows", CASES)
def test_fused_gradients_have_the_bits_of_the_chain(od, H, nh, rows, f64):
    c = case(od, H, nh, rows, f64)
    vclip = (H == 32) == (nh == 2)  # half of the shapes with the clipped value loss
    cfg = ppo.config(vf_clip=R.VF_CLIP if vclip else None)
    gp, gv, stats = fused(c, cfg, vclip)
    want_p, want_v = chain(c, cfg, vclip)
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all())
    assert float(want_p.abs().max()) > 0 and float(want_v.abs().max()) > 0
    assert torch.equal(ibits(gp), ibits(want_p)), "the policy's gradient"
    assert torch.equal(ibits(gv), ibits(want_v)), "the critic's gradient"
    ref = reference(c, vclip)
    assert not ref["undecided"].any(), "the case's inputs leave no row's branch to the last bits"
    got = stats.cpu().numpy()
    print(f"OD {od} H {H} layers {nh} rows {rows}: stats {got.tolist()} err {np.abs(got - ref['stats']).tolist()}")
    ok = R.stats_close(got, ref)
    assert ok.all(), f"stats {[R.STATS[i] for i in np.argwhere(~ok)[:, 0]]}: {got} vs {ref['stats']}"


def test_without_stats_the_gradients_keep_their_bits():
    c = case(6, 16, 2, 4097, False)
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    gp, gv, _ = fused(c, cfg, True)
    np_, nv, _ = fused(c, cfg, True, want_stats=False)
    assert torch.equal(ibits(np_), ibits(gp)) and torch.equal(ibits(nv), ibits(gv))


@pytest.mark.parametrize("which", ["policy", "critic"])
def test_either_net_may_be_left_out(which):
    c = case(6, 16, 2, 4097, False)
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    gp, gv, stats = fused(c, cfg, True)
    pol = which == "policy"
    hp, hv, half = fused(c, cfg, True, pol=pol, crit=not pol)
    s, h = stats.cpu().numpy(), half.cpu().numpy()
    if pol:
        assert torch.equal(ibits(hp), ibits(gp)) and bool(torch.isnan(hv).all()), "grad_value is not written"
        assert h[2] == 0.0 and np.array_equal(h[[1, 3, 4, 5, 6, 7]], s[[1, 3, 4, 5, 6, 7]])
        assert h[0] == h[1] - float(F32(0.01)) * h[3]
    else:
        assert torch.equal(ibits(hv), ibits(gv)) and bool(torch.isnan(hp).all()), "grad_policy is not written"
        assert h[2] == s[2] and not h[[1, 3, 4, 5, 6]].any() and h[7] == s[7] and h[0] == float(F32(0.5)) * h[2]


def test_ppo_grads_accumulates_as_a_backward_would():
    c = case.__wrapped__(4, 32, 2, 4097, False)  # nets of its own: it sets requires_grad and .grad on them
    pol, crit = c["pol"], c["crit"]
    cfg = ppo.config(vf_clip=R.VF_CLIP)
    gp, gv, stats = fused(c, cfg, True)
    args = (c["obs"], c["actions"], c["old_logp"], c["adv"], c["ret"])
    pol.params.requires_grad_(True)
    crit.params.requires_grad_(True)
    pol.params.grad = crit.params.grad = None
    s1 = ppo.ppo_grads(pol, crit, *args, old_values=c["old_values"], vf_clip=R.VF_CLIP)
    assert torch.equal(ibits(pol.params.grad), ibits(gp)) and torch.equal(ibits(crit.params.grad), ibits(gv))
    assert torch.equal(s1.view(torch.int64), stats.view(torch.int64))
    ppo.ppo_grads(pol, crit, *args, old_values=c["old_values"], vf_clip=R.VF_CLIP)
    assert torch.equal(ibits(pol.params.grad), ibits(gp + gp)) and torch.equal(ibits(crit.params.grad), ibits(gv + gv))
    # the same bits as the composed form under autograd
    pol.params.grad = crit.params.grad = None
    loss, s2 = ppo.ppo_loss(pol.forward(c["obs"]), crit.forward(c["obs"]), c["actions"], c["old_logp"], c["adv"],
                            c["ret"], old_values=c["old_values"], vf_clip=R.VF_CLIP)
    loss.backward()
    assert torch.equal(ibits(pol.params.grad), ibits(gp)) and torch.equal(ibits(crit.params.grad), ibits(gv))
    assert R.stats_close(s1.cpu().numpy(), reference(c, True)).all() and R.stats_close(s2.cpu().numpy(), reference(c, True)).all()
    pol.params.grad = crit.params.grad = None
    ppo.ppo_grads(pol, None, *args)
    assert crit.params.grad is None and torch.equal(ibits(pol.params.grad), ibits(gp))


def test_same_arguments_same_bits_on_any_stream():
    c = case(6, 32, 2, 70001, False)
    cfg = ppo.config()
    a = fused(c, cfg, False)
    b = fused(c, cfg, False)
    d = fused(c, cfg, False, stream=torch.cuda.Stream(DEV))
    for x, y, z in zip(a, b, d):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8), z.view(torch.uint8))


def test_zero_rows_writes_zeros():
    c = case(4, 16, 1, 1, False)
    cfg = ppo.config()
    gp = torch.full_like(c["pol"].params, float("nan"))
    gv = torch.full_like(c["crit"].params, float("nan"))
    stats = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
    _abi.check(_abi.lib().macm_ppo_grad(ctypes.byref(cfg), ctypes.byref(c["pol"].struct()), ctypes.byref(c["crit"].struct()),
                                        p(c["obs"]), 0, 0, p(c["actions"]), p(c["old_logp"]), p(c["adv"]), p(c["ret"]),
                                        None, p(gp), p(gv), p(stats), None, 0, None), "macm_ppo_grad")
    torch.cuda.synchronize()
    assert not gp.any() and not gv.any() and not stats.any()
