"""macm_policy_logp and macm_ppo_loss (csrc/ppo_loss.hip) through the C-ABI against tests/ppo_ref.py: row counts
around a wave, over several blocks and past the cap on the blocks (the grid-stride loop); with and without old
values, ent_coef = 0, logits-only and values-only calls, a scale pointer at 0.5; every subset of the outputs
(an output that is not wanted is NULL, and the others keep their bits). The inputs carry NaN rows after `rows`
(a lane that read past the end would show), the outputs start as the fill pattern and sit between guard
bands, as does the workspace. Tolerances: ppo_ref's (one float32 ulp or 2^-44 of the magnitude per element,
(rows + 64) 2^-52 of the magnitude per stat, clip_frac and rows exact); every row is compared, since
tests/test_ppo_ref.py asserts that none of these inputs' rows is undecided."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ppo_ref as R
from guard_bands import FILL, Guarded

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402
from gym_macm import ppo  # noqa: E402

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
TAIL = 70  # NaN rows behind the rows of a call
PAST_CAP = R.PAST_CAP  # more rows than the largest grid has threads: the second trip of the loop
VARIANTS = {
    "plain": dict(),
    "vclip": dict(vf_clip=R.VF_CLIP),
    "ent0": dict(ent_coef=0.0),
    "scale": dict(scale=0.5, vf_clip=R.VF_CLIP),
    "logits_only": dict(values=False),
    "values_only": dict(logits=False, vf_clip=R.VF_CLIP),
}
FLOATS = ("logits", "old_logp", "adv", "values", "ret", "old_values")


@functools.lru_cache(maxsize=None)
def inputs(rows):
    return R.inputs(rows)


@functools.lru_cache(maxsize=None)
def device_inputs(rows):
    x, out = inputs(rows), {}
    for name, a in x.items():
        full = np.full((rows + TAIL,) + a.shape[1:], np.nan if a.dtype == F32 else 7, a.dtype)
        full[:rows] = a
        out[name] = torch.from_numpy(full).to(DEV)
    return out


@functools.lru_cache(maxsize=None)
def reference(rows, variant):
    x, v = inputs(rows), dict(VARIANTS[variant])
    lg, vals = v.pop("logits", True), v.pop("values", True)
    return R.loss(x["logits"] if lg else None, x["actions"], x["old_logp"], x["adv"], x["values"] if vals else None,
                  x["ret"], x["old_values"] if "vf_clip" in v else None, **v)


def run_loss(rows, variant, want=("dlogits", "dvalues", "stats"), stream=None, n=None):
    """One macm_ppo_loss call into guarded buffers; a dict of numpy arrays (an output not wanted: None)"""
    v = dict(VARIANTS[variant])
    lg, vals = v.pop("logits", True), v.pop("values", True)
    scale = v.pop("scale", None)
    d = device_inputs(rows)
    cfg = ppo.config(v.get("clip", 0.2), v.get("vf_coef", 0.5), v.get("ent_coef", 0.01), v.get("vf_clip"))
    n = rows if n is None else n
    bufs = dict(dlogits=Guarded((rows, 9), torch.float32, DEV), dvalues=Guarded((rows,), torch.float32, DEV),
                stats=Guarded((8,), torch.float64, DEV))
    nbytes = ppo.workspace_bytes(n)
    ws = Guarded((max(nbytes, 16),), torch.uint8, DEV)
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV) if scale is not None else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    use = lambda name, on: p(d[name]) if on else None
    out = lambda name, on: p(bufs[name].t) if (name in want and on) else None
    torch.cuda.synchronize()
    _abi.check(_abi.lib().macm_ppo_loss(
        ctypes.byref(cfg), n, use("logits", lg), use("actions", lg), use("old_logp", lg), use("adv", lg),
        use("values", vals), use("ret", vals), use("old_values", vals and "vf_clip" in v), p(sc), out("dlogits", lg),
        out("dvalues", vals), out("stats", True), p(ws.t) if nbytes else None, nbytes,
        ctypes.c_void_p(stream.cuda_stream) if stream is not None else None), "macm_ppo_loss")
    torch.cuda.synchronize()
    res = {}
    for name, g in bufs.items():
        assert g.bands_intact(), f"a store outside {name}"
        written = name in want and (name == "stats" or (lg if name == "dlogits" else vals))
        if not written or (n == 0 and name != "stats"):
            assert bool((g.bytes == FILL).all()), f"{name} was not wanted and was written"
            res[name] = None
        else:
            res[name] = g.t.cpu().numpy()
    assert ws.bands_intact(), "a store outside the workspace"
    return res


def check(got, ref, rows, ctx):
    if got["dlogits"] is not None:
        ok = R.close(got["dlogits"], ref["dlogits"], ref["S_dlogits"])
        assert np.isfinite(got["dlogits"]).all() and ok.all(), f"{ctx}: dlogits, {np.argwhere(~ok)[:3].tolist()}"
    if got["dvalues"] is not None:
        ok = R.close(got["dvalues"], ref["dvalues"], ref["S_dvalues"])
        assert np.isfinite(got["dvalues"]).all() and ok.all(), f"{ctx}: dvalues, rows {np.argwhere(~ok)[:3].tolist()}"
    if got["stats"] is not None:
        err = np.abs(got["stats"] - ref["stats"])
        print(ctx, "stats", got["stats"].tolist(), "err", err.tolist())
        ok = R.stats_close(got["stats"], ref)
        assert ok.all(), f"{ctx}: stats {[R.STATS[i] for i in np.argwhere(~ok)[:, 0]]}: {got['stats']} vs {ref['stats']}"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("rows", R.ROWS)
def test_ppo_loss_against_the_reference(rows, variant):
    ref = reference(rows, variant)
    got = run_loss(rows, variant)
    check(got, ref, rows, f"rows {rows} {variant}")
    if rows >= 63 and VARIANTS[variant].get("logits", True):
        assert np.count_nonzero(got["dlogits"]) > rows and (np.abs(inputs(rows)["logits"]) == 80).any()


def test_ppo_loss_past_the_cap_on_the_blocks():
    check(run_loss(PAST_CAP, "vclip"), reference(PAST_CAP, "vclip"), PAST_CAP, "past the cap")


@pytest.mark.parametrize("want", [("stats",), ("dlogits",), ("dvalues",), ("dlogits", "dvalues"), ()])
def test_an_output_that_is_not_wanted_is_not_written_and_the_others_keep_their_bits(want):
    rows = 4097
    full = run_loss(rows, "vclip")
    got = run_loss(rows, "vclip", want=want)
    for name in ("dlogits", "dvalues", "stats"):
        if name in want:
            assert np.array_equal(got[name].view(np.uint8), full[name].view(np.uint8)), name
        else:
            assert got[name] is None


def test_zero_rows_zeros_the_stats_and_touches_nothing_else():
    got = run_loss(65, "vclip", n=0)  # no workspace: NULL, 0 bytes
    assert got["dlogits"] is None and got["dvalues"] is None
    assert np.array_equal(got["stats"].view(np.uint64), np.zeros(8, np.uint64))


def test_same_arguments_same_bits_on_any_stream():
    rows = 131137
    a = run_loss(rows, "vclip")
    b = run_loss(rows, "vclip")
    c = run_loss(rows, "vclip", stream=torch.cuda.Stream(DEV))
    for name in ("dlogits", "dvalues", "stats"):
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
        assert np.array_equal(a[name].view(np.uint8), c[name].view(np.uint8)), name


@pytest.mark.parametrize("with_entropy", [True, False], ids=["entropy", "no_entropy"])
@pytest.mark.parametrize("rows", R.ROWS)
def test_policy_logp_against_the_reference(rows, with_entropy):
    x, d = inputs(rows), device_inputs(rows)
    logp, H, S = R.log_prob(x["logits"], x["actions"])
    p, lp, _, _ = R.heads(x["logits"], x["actions"])
    g_lp, g_H = Guarded((rows,), torch.float32, DEV), Guarded((rows,), torch.float32, DEV)
    torch.cuda.synchronize()
    _abi.check(_abi.lib().macm_policy_logp(ctypes.c_void_p(d["logits"].data_ptr()), ctypes.c_void_p(d["actions"].data_ptr()),
                                           rows, ctypes.c_void_p(g_lp.t.data_ptr()),
                                           ctypes.c_void_p(g_H.t.data_ptr()) if with_entropy else None, None),
               "macm_policy_logp")
    torch.cuda.synchronize()
    assert g_lp.bands_intact() and g_H.bands_intact()
    got = g_lp.t.cpu().numpy()
    assert np.isfinite(got).all() and R.close(got, logp, S).all()
    if with_entropy:  # the magnitude of H: the sum of |p lp| over the row's nine terms
        gH = g_H.t.cpu().numpy()
        assert np.isfinite(gH).all() and R.close(gH, H, np.abs(p * lp).sum(axis=(1, 2))).all()
    else:
        assert bool((g_H.bytes == FILL).all())
    # the Python wrapper gives the same bits, and old_logp from these logits makes the ratio exactly 1
    t = ppo.log_prob(d["logits"][:rows], d["actions"][:rows])
    assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32))
    _, stats = ppo.ppo_loss(d["logits"][:rows], None, d["actions"][:rows], t, d["adv"][:rows], None)
    s = stats.cpu().numpy()
    assert s[4] == 0.0 and s[5] == 0.0 and s[6] == 1.0 and s[7] == rows
