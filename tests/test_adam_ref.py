"""tests/adam_ref.py, the numpy restatement of macm_ppo_adam (include/macm.h), without a GPU.

Its float64-state mode is Adam behind clip_grad_norm_ in double and is held against torch.optim.Adam
(float64 params, foreach=False) with torch.nn.utils.clip_grad_norm_: 10 steps on the smallest net pair
(4 -> 16 -> 9 and 4 -> 16 -> 1: 233 + 97 params) and on the largest (6 -> 32 -> 32 -> 9 and 6 -> 32 -> 32 -> 1:
1,577 + 1,313), gradient norms on both sides of max_grad_norm. Both are the same real function with about ten
float64 roundings per step, each of relative size 2^-53 on quantities of the size of the update (lr = 1e-2
here) or of the norm, so after 10 steps they agree far inside 1e-12 max(1, |param|). Three deliberately
wrong references (eps inside the root, no bias correction, the clip without its 1e-6) must each fail that
comparison at the same inputs: the tolerance separates them. The smallest of the three differences is the
clip's: a relative 1e-6 / norm in the gradient of the clipped steps, which reaches the params through the
mix of clipped and unclipped steps in m and v, some 1e-9 at this lr.

The float32-state mode (the device's) gives the same bits on every run, a zero state is a fresh optimiser,
and the gate, the non-finite skip and resume behave as the header says."""
import numpy as np
import pytest
import torch

import adam_ref as A

PAIRS = {"smallest": (4, 16, 1), "largest": (6, 32, 2)}
SCALES = (0.3, 0.5, 0.8, 2.0, 3.0, 0.4, 5.0, 0.9, 1.5, 0.2)  # gradient norms around max_grad_norm = 1
CFG = A.Cfg(lr=1e-2, max_grad_norm=1.0)
TOL = 1e-12


def counts(od, H, nh):
    trunk = od * H + H + (H * H + H if nh == 2 else 0)
    return trunk + H * 9 + 9, trunk + H + 1


def draws(name, dtype):
    n_p, n_c = counts(*PAIRS[name])
    rng = np.random.default_rng([77, n_p])
    params = [(0.5 * rng.standard_normal(n)).astype(dtype) for n in (n_p, n_c)]
    grads = []
    for s in SCALES:
        g = rng.standard_normal(n_p + n_c)
        g = (g * (s / np.linalg.norm(g))).astype(dtype)
        grads.append([g[:n_p].copy(), g[n_p:].copy()])
    return params, grads


def run_ref(params, grads, cfg, dtype, variant=None, st=None):
    params = [p.copy() for p in params]
    st = A.zero_state(params[0].size, params[1].size, dtype) if st is None else st
    coefs = []
    for g in grads:
        assert A.step(params, g, st, cfg, variant=variant) == "step"
        coefs.append(float(st["head"][5]))
    return params, st, coefs


def run_torch(params, grads, cfg):
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = torch.optim.Adam(ps, lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps, foreach=False)
    for g in grads:
        for p, gi in zip(ps, g):
            p.grad = torch.from_numpy(gi.copy())
        torch.nn.utils.clip_grad_norm_(ps, cfg.max_grad_norm, foreach=False)
        opt.step()
    return [p.detach().numpy() for p in ps]


def worst(got, want):
    """The largest |got - want| / max(1, |want|) over both nets"""
    return max(float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(PAIRS))
def test_float64_mode_is_torch_adam_behind_clip_grad_norm(name):
    params, grads = draws(name, np.float64)
    assert (params[0].size, params[1].size) == ((233, 97) if name == "smallest" else (1577, 1313))
    want = run_torch(params, grads, CFG)
    got, st, coefs = run_ref(params, grads, CFG, np.float64)
    assert sum(c < 1.0 for c in coefs) >= 3 and sum(c == 1.0 for c in coefs) >= 3, "clipping on some steps, off on others"
    assert st["head"][0] == len(SCALES)
    err = worst(got, want)
    print(f"{name}: reference against torch {err:.3e}")
    assert err <= TOL
    for variant in A.VARIANTS:
        bad, _, _ = run_ref(params, grads, CFG, np.float64, variant=variant)
        e = worst(bad, want)
        print(f"{name}: {variant} against torch {e:.3e}")
        assert e > TOL, f"the tolerance does not tell {variant} from the definition"


@pytest.mark.parametrize("name", list(PAIRS))
def test_float32_mode_is_deterministic_and_near_float64(name):
    params, grads = draws(name, np.float32)
    a, sa, _ = run_ref(params, grads, CFG, np.float32)
    b, sb, _ = run_ref(params, grads, CFG, np.float32)
    assert all(x.dtype == np.float32 for x in a + sa["m"] + sa["v"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and A.state_bytes(sa) == A.state_bytes(sb)
    # an explicitly initialised state (t = 0, both powers 1) is the zero state
    c, sc, _ = run_ref(params, grads, CFG, np.float32, st=A.init_state(params[0].size, params[1].size))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c)) and A.state_bytes(sa) == A.state_bytes(sc)
    # float32 storage: each step rounds the params once (2^-24 relative) and m, v likewise
    wide, _, _ = run_ref([p.astype(np.float64) for p in params], [[g.astype(np.float64) for g in gs] for gs in grads],
                         CFG, np.float64)
    assert worst(a, wide) < 1e-5 and not all(np.array_equal(x, y) for x, y in zip(a, params))
    assert len(A.state_bytes(sa)) == 64 + 8 * (params[0].size + params[1].size)


def test_powers_are_running_products():
    params, grads = draws("smallest", np.float32)
    _, st, _ = run_ref(params, grads[:3], A.Cfg(), np.float32)
    assert st["head"][1] == (np.float64(0.9) * 0.9) * 0.9 and st["head"][2] == (np.float64(0.999) * 0.999) * 0.999
    assert st["head"][0] == 3.0 and st["head"][3] == 0.0 and st["head"][6] == 0.0 and st["head"][7] == 0.0


def test_gate_skip_and_resume():
    params, grads = draws("smallest", np.float32)
    cfg = A.Cfg(lr=1e-2, max_grad_norm=1.0, target_kl=0.02)
    p = [x.copy() for x in params]
    st = A.zero_state(p[0].size, p[1].size)
    stats = np.zeros(8)
    stats[4] = 0.02  # equal to the target: not above it
    assert A.step(p, grads[0], st, cfg, stats=stats) == "step"
    before = ([x.copy() for x in p], A.copy_state(st))

    def unchanged(but=()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(p, before[0]))
        for k in range(8):
            assert k in but or st["head"][k] == before[1]["head"][k]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(st["m"] + st["v"], before[1]["m"] + before[1]["v"]))

    # a gradient that is not finite: counted, nothing else moves
    for bad, n in ((np.nan, 1.0), (np.inf, 2.0)):
        g = [grads[1][0].copy(), grads[1][1].copy()]
        g[1][5] = bad
        assert A.step(p, g, st, cfg, stats=stats) == "skip"
        assert st["head"][6] == n and not np.isfinite(st["head"][4])
        unchanged(but=(4, 6))
    before = ([x.copy() for x in p], A.copy_state(st))
    # approx_kl over the target, or NaN: stopped, and a low KL afterwards does not reopen it
    for kl in (0.0200001, np.nan):
        s = A.copy_state(st)
        hi = stats.copy()
        hi[4] = kl
        q = [x.copy() for x in p]
        assert A.step(q, grads[1], s, cfg, stats=hi) == "stop" and s["head"][3] == 1.0
    hi = stats.copy()
    hi[4] = 1.0
    assert A.step(p, grads[1], st, cfg, stats=hi) == "stop"
    unchanged(but=(3,))
    assert A.step(p, grads[1], st, cfg, stats=stats) == "stopped"
    unchanged(but=(3,))
    A.resume(st)
    assert A.step(p, grads[1], st, cfg, stats=stats) == "step" and st["head"][0] == 2.0
    # no target, or no stats: no gate
    assert A.step(p, grads[2], st, A.Cfg(target_kl=0.0), stats=hi) == "step"
    assert A.step(p, grads[2], st, cfg, stats=None) == "step"


def test_norm_association_and_clip_edges():
    rng = np.random.default_rng(5)
    g = rng.standard_normal(330).astype(np.float32)
    s = np.zeros(256)
    for j, x in enumerate(g):  # element j belongs to thread j mod 256, ascending j
        s[j % 256] = s[j % 256] + np.float64(x) * np.float64(x)
    d = 128
    while d:
        for i in range(d):
            s[i] = s[i] + s[i + d]
        d //= 2
    assert A.grad_norm([g[:233], g[233:]]) == np.sqrt(s[0])
    # max_grad_norm = 0: no clipping; a zero gradient: norm 0, coef 1 (max / 1e-6 is above 1), params unmoved at m = v = 0
    for cfg, gs, coef in ((A.Cfg(max_grad_norm=0.0), [g[:233], g[233:]], 1.0),
                          (A.Cfg(max_grad_norm=1.0), [np.zeros(233, np.float32), np.zeros(97, np.float32)], 1.0)):
        p = [np.ones(233, np.float32), np.ones(97, np.float32)]
        st = A.zero_state(233, 97)
        assert A.step(p, gs, st, cfg) == "step" and st["head"][5] == coef
    assert st["head"][4] == 0.0 and all(np.array_equal(x, np.ones_like(x)) for x in p)
