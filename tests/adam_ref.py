"""macm_ppo_adam in numpy (a helper, not a test): the definition of include/macm.h restated with float64
operations, each rounded once, in the header's association: + - * / sqrt only, which numpy computes with the
bits the device computes. What is stored as float32 is one rounding of a float64.

    st = zero_state(n_p, n_c)                      # an all-zero state is a fresh optimiser
    step([pp, pc], [gp, gc], st, Cfg(lr=...))      # params and st change in place; returns what happened

params and grads are [policy, critic]; a net that is absent is an empty array. dtype float32 is the device's
mode. With dtype float64 (zero_state(..., np.float64), float64 params and gradients) the roundings to float32
disappear and the function is plain Adam behind clip_grad_norm_ in double, which tests/test_adam_ref.py holds
against torch. `variant` selects one of three deliberately wrong definitions that the same comparison must
tell apart."""
import dataclasses

import numpy as np

BLOCK = 256
HEAD = ("t", "p1", "p2", "stopped", "norm", "coef", "skipped", "zero")
VARIANTS = ("eps_in_root", "no_bias_correction", "clip_without_1e-6")
F64 = np.float64


@dataclasses.dataclass
class Cfg:
    lr: float = 3e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    max_grad_norm: float = 0.0
    target_kl: float = 0.0


def zero_state(n_p, n_c, dtype=np.float32):
    z = lambda n: np.zeros(n, dtype)
    return dict(head=np.zeros(8, F64), m=[z(n_p), z(n_c)], v=[z(n_p), z(n_c)])


def init_state(n_p, n_c, dtype=np.float32):
    """The same optimiser written out: t = 0 with both powers 1 (the kernel takes them as 1 at t = 0)"""
    st = zero_state(n_p, n_c, dtype)
    st["head"][1] = st["head"][2] = 1.0
    return st


def copy_state(st):
    return dict(head=st["head"].copy(), m=[a.copy() for a in st["m"]], v=[a.copy() for a in st["v"]])


def state_bytes(st):
    """The device layout: double head[8], then m and v of the policy, then of the critic"""
    return b"".join(a.tobytes() for a in (st["head"], st["m"][0], st["v"][0], st["m"][1], st["v"][1]))


def grad_norm(grads):
    """sqrt of the sum of squares in the kernel's association: thread i sums its elements i, i + 256, ... in
    ascending order from 0, then s[i] += s[i + d] for d = 128 .. 1"""
    g = np.concatenate([np.asarray(a).astype(F64) for a in grads])
    pad = np.zeros(-(-max(g.size, 1) // BLOCK) * BLOCK, F64)  # a thread past the end adds + 0.0: exact
    pad[:g.size] = g
    s = np.zeros(BLOCK, F64)
    for row in pad.reshape(-1, BLOCK):
        s = s + row * row
    d = BLOCK // 2
    while d >= 1:
        s[:d] = s[:d] + s[d:2 * d]
        d //= 2
    return np.sqrt(s[0])


def step(params, grads, st, cfg, stats=None, variant=None):
    """One macm_ppo_adam call; returns "stopped" (already), "stop" (the gate closed now), "skip" (a norm that is
    not finite) or "step"."""
    assert variant is None or variant in VARIANTS
    head = st["head"]
    if head[3] != 0.0:
        return "stopped"
    if stats is not None and cfg.target_kl > 0.0 and not (stats[4] <= cfg.target_kl):
        head[3] = 1.0
        return "stop"
    with np.errstate(all="ignore"):
        norm = grad_norm(grads)
    if not np.isfinite(norm):
        head[6] = head[6] + 1.0
        head[4] = norm
        return "skip"
    coef = F64(1.0)
    if cfg.max_grad_norm > 0.0:
        c = F64(cfg.max_grad_norm) / (norm if variant == "clip_without_1e-6" else norm + F64(1e-6))
        coef = c if c < 1.0 else F64(1.0)
    b1, b2, lr, eps = F64(cfg.beta1), F64(cfg.beta2), F64(cfg.lr), F64(cfg.eps)
    omb1, omb2 = F64(1.0) - b1, F64(1.0) - b2
    t = head[0]
    p1 = (F64(1.0) if t == 0.0 else head[1]) * b1
    p2 = (F64(1.0) if t == 0.0 else head[2]) * b2
    c1, c2 = (F64(1.0), F64(1.0)) if variant == "no_bias_correction" else (F64(1.0) - p1, F64(1.0) - p2)
    for w in range(2):
        dt = st["m"][w].dtype
        g = np.asarray(grads[w]).astype(F64) * coef
        m = (b1 * st["m"][w].astype(F64) + omb1 * g).astype(dt)
        v = (b2 * st["v"][w].astype(F64) + omb2 * (g * g)).astype(dt)
        if variant == "eps_in_root":
            den = np.sqrt(v.astype(F64) / c2 + eps)
        else:
            den = np.sqrt(v.astype(F64) / c2) + eps
        st["m"][w], st["v"][w] = m, v
        params[w][...] = (params[w].astype(F64) - lr * ((m.astype(F64) / c1) / den)).astype(params[w].dtype)
    head[0], head[1], head[2], head[4], head[5] = t + 1.0, p1, p2, norm, coef
    return "step"


def resume(st):
    st["head"][3] = 0.0
