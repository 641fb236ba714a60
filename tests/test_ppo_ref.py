"""tests/ppo_ref.py, the numpy float64 statement of the PPO loss (include/macm.h, macm_ppo_loss), without a GPU:
against torch.autograd in float64 on the loss of tools/grad_bench.py (and its clipped-value variant), each
element to 1e-12 of its magnitude (ppo_ref's S and stat_mag: the sizes of the terms it is summed from, which
is looser than 1e-12 of the value where they cancel, and is what float64 rounding of those terms can reach), the
first-epoch identities (ratio exactly 1, approx_kl 0, clip_frac 0, g_logp = -adv), saturated and tied logits,
and the condition the GPU tests rest on: none of their seeded rows is undecided."""
import numpy as np
import pytest
import torch

import ppo_ref as R

F32, F64 = np.float32, np.float64


def torch_loss(x, rows, clip, vf_coef, ent_coef, vf_clip):
    """grad_bench.py's ppo_loss in float64 with old_logp given; logp goes through float32 with the identity as
    its derivative, as the definition says. Returns (loss, logits, values) with .grad set."""
    t = lambda a: torch.from_numpy(np.asarray(a, F32).astype(F64))
    lg = t(x["logits"][:rows]).requires_grad_(True)
    v = t(x["values"][:rows]).requires_grad_(True)
    lp = torch.log_softmax(lg.view(rows, 3, 3), -1)
    a = torch.from_numpy(x["actions"][:rows].astype(np.int64)).unsqueeze(-1)
    logp = lp.gather(-1, a).squeeze(-1).sum(-1)
    logp = logp + (logp.detach().float().double() - logp.detach())
    ratio = torch.exp(logp - t(x["old_logp"][:rows]))
    adv, ret = t(x["adv"][:rows]), t(x["ret"][:rows])
    eps = float(F32(clip))
    pg = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - eps, 1 + eps) * adv).mean()
    if vf_clip is None:
        vloss = 0.5 * ((v - ret) ** 2).mean()
    else:
        ov, ev = t(x["old_values"][:rows]), float(F32(vf_clip))
        vc = ov + torch.clamp(v - ov, -ev, ev)
        vloss = 0.5 * torch.maximum((v - ret) ** 2, (vc - ret) ** 2).mean()
    entropy = -(lp.exp() * lp).sum((-1, -2)).mean()
    loss = pg + float(F32(vf_coef)) * vloss - float(F32(ent_coef)) * entropy
    loss.backward()
    return loss, lg, v


def ref_of(x, rows, **kw):
    old = x["old_values"][:rows] if kw.get("vf_clip") is not None else None
    return R.loss(x["logits"][:rows], x["actions"][:rows], x["old_logp"][:rows], x["adv"][:rows], x["values"][:rows],
                  x["ret"][:rows], old, **kw)


@pytest.mark.parametrize("cfg", [dict(), dict(vf_clip=R.VF_CLIP), dict(ent_coef=0.0), dict(vf_coef=0.0),
                                 dict(clip=0.1, vf_coef=1.0, ent_coef=0.05, vf_clip=0.5)],
                         ids=["default", "vclip", "ent0", "vf0", "other"])
@pytest.mark.parametrize("rows", [1, 65, 4097])
def test_reference_against_torch_autograd(rows, cfg):
    x = R.inputs(4097)
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, vf_clip=None)
    kw.update(cfg)
    ref = ref_of(x, rows, **kw)
    loss, lg, v = torch_loss(x, rows, **kw)
    assert not ref["undecided"].any()
    assert abs(float(loss.detach()) - ref["stats"][0]) <= 1e-12 * ref["stat_mag"][0]
    assert np.all(np.abs(lg.grad.numpy() - ref["dlogits"]) <= 1e-12 * ref["S_dlogits"])
    assert np.all(np.abs(v.grad.numpy() - ref["dvalues"]) <= 1e-12 * np.maximum(ref["S_dvalues"], 1e-300))
    assert np.abs(ref["dlogits"]).max() > 0 and (kw["vf_coef"] == 0 or np.abs(ref["dvalues"]).max() > 0)


@pytest.mark.parametrize("rows", [1, 65, 4097])
def test_first_epoch_identities(rows):
    x = R.inputs(rows)
    logp, H, _ = R.log_prob(x["logits"], x["actions"])
    ref = R.loss(x["logits"], x["actions"], logp.astype(F32), x["adv"], clip=0.2)
    assert np.all(ref["ratio"] == 1.0)
    assert ref["stats"][4] == 0.0 and ref["stats"][5] == 0.0 and ref["stats"][6] == 1.0
    assert np.array_equal(ref["g_logp"], -x["adv"].astype(F64))
    assert ref["stats"][7] == rows and np.isfinite(H).all()


def test_saturated_and_tied_logits_stay_finite():
    z = np.array([[80, -80, 80, -80, -80, -80, 80, 80, 80], [-80] * 9, [0.75] * 9, [80, 0, -80, 1, 1, 1, -80, 80, 0]], F32)
    a = np.array([[1, 2, 0], [0, 1, 2], [2, 2, 2], [2, 0, 0]], np.uint8)
    logp, H, _ = R.log_prob(z, a)
    assert np.isfinite(logp).all() and np.isfinite(H).all()
    assert logp[2] == 3 * np.log(1 / 3) or abs(logp[2] - 3 * np.log(1 / 3)) < 1e-15
    ref = R.loss(z, a, logp.astype(F32), np.ones(4, F32), np.zeros(4, F32), np.ones(4, F32))
    for key in ("dlogits", "dvalues", "stats"):
        assert np.isfinite(ref[key]).all(), key
    x = R.inputs(4097)
    assert (np.abs(x["logits"]) == 80).any() and np.isfinite(ref_of(x, 4097, vf_clip=R.VF_CLIP)["dlogits"]).all()


@pytest.mark.parametrize("rows", R.ROWS + (R.PAST_CAP,))
def test_the_seeded_inputs_have_no_undecided_row(rows):
    """A condition, not a tolerance: the GPU tests compare every row of these inputs."""
    x = R.inputs(rows)
    for kw in (dict(), dict(vf_clip=R.VF_CLIP), dict(ent_coef=0.0), dict(scale=0.5)):
        ref = ref_of(x, rows, **kw)
        assert int(ref["undecided"].sum()) == 0
    if rows >= 4097:  # both branches of every comparison occur
        ref = ref_of(x, rows, vf_clip=R.VF_CLIP)
        assert 0 < ref["stats"][5] < 1 and (ref["g_logp"] == 0).any() and (ref["dvalues"] == 0).any()


def test_close_and_stats_close_refuse_what_they_must():
    want, S = np.array([1.0, 1e-3, 0.0]), np.array([1.0, 1.0, 1.0])
    assert R.close(want.astype(F32), want, S).all()
    assert R.close(np.nextafter(want.astype(F32), F32(2)), want, S).all()
    assert not R.close((want + 1e-5).astype(F32), want, S).any()
    ref = dict(rows=10, stats=np.arange(8.0), stat_mag=np.ones(8))
    assert R.stats_close(np.arange(8.0), ref).all()
    assert not R.stats_close(np.arange(8.0) + 1e-9, ref).any()
