"""macm_ppo_adam (csrc/ppo_adam.hip) against tests/adam_ref.py, bit for bit in the params, m, v and all eight
head words after every call: the smallest net pair (233 + 97 elements: threads with one and with two
elements), the largest (1,577 + 1,313), the policy alone and the critic alone; successive steps from a zero
state (the powers and the bias correction); gradient norms below, above and equal to max_grad_norm, no
clipping, an all-zero gradient; a NaN and an inf element (nothing moves but the count and the norm); the KL
gate (over the target, NaN, a no-op until the stopped word is cleared); lr changed between calls. Params,
state, gradients and stats sit between guard bands; the gradients and stats are inputs and keep their bits."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref as A
from guard_bands import Guarded
from test_adam_ref import counts

pytestmark = pytest.mark.gpu

from gym_macm import _abi  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
SHAPES = {"smallest": ((4, 16, 1), True, True), "largest": ((6, 32, 2), True, True),
          "policy_alone": ((4, 32, 2), True, False), "critic_alone": ((4, 32, 1), False, True)}


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Twin:
    """One optimiser on the device (guarded buffers, macm_ppo_adam through ctypes) and in adam_ref"""

    def __init__(self, name, seed=0):
        (od, H, nh), pol, crit = SHAPES[name]
        n_p, n_c = counts(od, H, nh)
        self.n = [n_p if pol else 0, n_c if crit else 0]
        rng = np.random.default_rng([8800, seed, n_p])
        self.rng = rng
        self.params = [(0.5 * rng.standard_normal(n)).astype(F32) for n in self.n]
        self.st = A.zero_state(*self.n)
        self.dparams = [Guarded((max(n, 1),), torch.float32, DEV) for n in self.n]  # (an absent net: one element, never passed)
        self.dgrads = [Guarded((max(n, 1),), torch.float32, DEV) for n in self.n]
        self.dstats = Guarded((8,), torch.float64, DEV)
        self.nbytes = 64 + 8 * sum(self.n)
        self.dstate = Guarded((self.nbytes,), torch.uint8, DEV)
        self.dstate.t.zero_()
        for d, a in zip(self.dparams, self.params):
            d.t[:a.size].copy_(torch.from_numpy(a))
        self.pol = _abi.MacmPolicyMlp(od, H, nh, 0, p(self.dparams[0].t)) if pol else None
        self.crit = _abi.MacmValueMlp(od, H, nh, 0, p(self.dparams[1].t)) if crit else None
        n = ctypes.c_int64(0)
        _abi.check(_abi.lib().macm_ppo_adam_state_bytes(self.ref(self.pol), self.ref(self.crit), ctypes.byref(n)),
                   "macm_ppo_adam_state_bytes")
        assert n.value == self.nbytes

    @staticmethod
    def ref(s):
        return ctypes.byref(s) if s is not None else None

    def grads(self, norm):
        """A gradient of both nets with about that norm (float32 rounding moves it in the last bits)"""
        g = self.rng.standard_normal(sum(self.n))
        g = (g * (norm / np.linalg.norm(g))).astype(F32)
        return [g[:self.n[0]].copy(), g[self.n[0]:].copy()]

    def head(self):
        return self.dstate.t[:64].view(torch.float64).cpu().numpy()

    def step(self, grads, cfg, stats=None, what=""):
        """The same call on both sides, then every bit compared; returns adam_ref's verdict"""
        for d, g in zip(self.dgrads, grads):
            d.t[:g.size].copy_(torch.from_numpy(g))
        if stats is not None:
            self.dstats.t.copy_(torch.from_numpy(np.asarray(stats, np.float64)))
        c = _abi.MacmAdamConfig(cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.max_grad_norm, cfg.target_kl,
                                (ctypes.c_int32 * 4)(0, 0, 0, 0))
        torch.cuda.synchronize()
        _abi.check(_abi.lib().macm_ppo_adam(
            ctypes.byref(c), self.ref(self.pol), self.ref(self.crit), p(self.dgrads[0].t) if self.pol else None,
            p(self.dgrads[1].t) if self.crit else None, p(self.dstats.t) if stats is not None else None,
            p(self.dstate.t), self.nbytes, None), "macm_ppo_adam")
        torch.cuda.synchronize()
        verdict = A.step(self.params, grads, self.st, cfg, stats=stats)
        for name, g in (("params", self.dparams), ("grads", self.dgrads), ("stats", [self.dstats]), ("state", [self.dstate])):
            assert all(x.bands_intact() for x in g), f"{what}: a store outside {name}"
        for d, g in zip(self.dgrads, grads):
            assert d.t[:g.size].cpu().numpy().tobytes() == g.tobytes(), f"{what}: the gradient was modified"
        if stats is not None:
            assert self.dstats.t.cpu().numpy().tobytes() == np.asarray(stats, np.float64).tobytes(), f"{what}: stats was modified"
        self.same(what)
        return verdict

    def same(self, what):
        head, ref = self.head(), self.st["head"]
        for k, name in enumerate(A.HEAD):
            assert head[k:k + 1].tobytes() == ref[k:k + 1].tobytes(), f"{what}: head[{k}] ({name}) {head[k]!r} != {ref[k]!r}"
        got = self.dstate.t.cpu().numpy().tobytes()
        want = A.state_bytes(self.st)
        assert len(got) == len(want) and got == want, f"{what}: m / v differ from the reference's bits"
        for w, (d, a) in enumerate(zip(self.dparams, self.params)):
            assert d.t[:a.size].cpu().numpy().tobytes() == a.tobytes(), f"{what}: the {'policy' if w == 0 else 'critic'}'s params differ"

    def resume(self):
        self.dstate.t[:64].view(torch.float64)[3:4].zero_()
        A.resume(self.st)


@pytest.mark.parametrize("name", list(SHAPES))
def test_successive_steps_from_a_zero_state(name):
    t = Twin(name)
    cfg = A.Cfg(lr=1e-2, max_grad_norm=1.0)
    before = [a.copy() for a in t.params]
    coefs = []
    for k, norm in enumerate((0.5, 2.0, 0.9)):  # below, above, below the clip
        if k == 2:
            cfg = A.Cfg(lr=3e-3, max_grad_norm=1.0)  # a schedule: lr changed between calls
        assert t.step(t.grads(norm), cfg, what=f"{name} step {k + 1}") == "step"
        coefs.append(t.st["head"][5])
    head = t.head()
    assert head[0] == 3.0 and head[1] == (0.9 * 0.9) * 0.9 and head[3] == 0.0 and head[6] == 0.0 and head[7] == 0.0
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0
    for a, b, n in zip(t.params, before, t.n):
        assert n == 0 or float(np.max(np.abs(a - b))) > 1e-3, "the params moved"


@pytest.mark.parametrize("name", ["smallest", "largest"])
def test_clip_edges(name):
    t = Twin(name, seed=1)
    one = [np.zeros(n, F32) for n in t.n]
    one[1][t.n[1] - 1] = 1.0  # norm = 1 exactly, in the last element of all
    zero = [np.zeros(n, F32) for n in t.n]
    for what, grads, mgn, coef in (("norm below", t.grads(0.25), 1.0, 1.0), ("norm above", t.grads(7.0), 1.0, None),
                                   ("norm equal", one, 1.0, 1.0 / (1.0 + 1e-6)), ("no clipping", t.grads(7.0), 0.0, 1.0),
                                   ("zero gradient", zero, 1.0, 1.0), ("zero gradient, no clipping", zero, 0.0, 1.0)):
        assert t.step(grads, A.Cfg(lr=1e-2, max_grad_norm=mgn), what=f"{name} {what}") == "step"
        head = t.head()
        assert coef is None or head[5] == coef, (what, head[5])
        assert coef is not None or 0.1 < head[5] < 0.2, (what, head[5])
        assert what != "norm equal" or head[4] == 1.0
        assert not what.startswith("zero") or head[4] == 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_nonfinite_gradients_are_skipped(name):
    t = Twin(name, seed=2)
    cfg = A.Cfg(lr=1e-2, max_grad_norm=1.0)
    assert t.step(t.grads(2.0), cfg, what="first") == "step"
    params, st = [a.copy() for a in t.params], A.copy_state(t.st)
    w = 0 if t.n[0] else 1
    for count, (bad, at) in enumerate(((np.nan, 0), (np.inf, t.n[w] - 1), (-np.inf, 300 % t.n[w])), 1):
        g = t.grads(2.0)
        g[w][at] = bad
        assert t.step(g, cfg, what=f"{name} {bad}") == "skip"
        head = t.head()
        assert head[6] == count and not np.isfinite(head[4])
        assert bool(np.isnan(head[4])) == bool(np.isnan(bad))
        # params, m, v, t and the powers keep their bits (the reference, which the device equals, did not move)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(t.params, params))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(t.st["m"] + t.st["v"], st["m"] + st["v"]))
        assert t.st["head"][:4].tobytes() == st["head"][:4].tobytes() and t.st["head"][5] == st["head"][5]
    assert t.step(t.grads(0.5), cfg, what="after") == "step" and t.head()[0] == 2.0 and t.head()[6] == 3.0


@pytest.mark.parametrize("name", ["smallest", "policy_alone"])
def test_kl_gate(name):
    cfg = A.Cfg(lr=1e-2, max_grad_norm=1.0, target_kl=0.02)
    stats = lambda kl: np.array([0.1, 0.2, 0.3, 0.4, kl, 0.0, 1.5, 4096.0])
    for over in (0.020001, 1.0, np.nan, np.inf):
        t = Twin(name, seed=3)
        assert t.step(t.grads(2.0), cfg, stats=stats(0.02), what="at the target") == "step"  # equal: not over
        assert t.step(t.grads(2.0), cfg, stats=stats(0.0), what="below") == "step"
        params, st = [a.copy() for a in t.params], A.copy_state(t.st)
        assert t.step(t.grads(2.0), cfg, stats=stats(over), what=f"kl {over}") == "stop"
        assert t.head()[3] == 1.0
        assert t.step(t.grads(2.0), cfg, stats=stats(0.0), what="stopped, low kl") == "stopped"
        assert t.step(t.grads(2.0), A.Cfg(lr=1e-2, max_grad_norm=1.0), what="stopped, no target and no stats") == "stopped"
        bad = t.grads(2.0)
        bad[0][0] = np.nan
        assert t.step(bad, cfg, stats=stats(0.0), what="stopped, NaN gradient") == "stopped"
        st["head"][3] = 1.0
        assert A.state_bytes(t.st) == A.state_bytes(st) and all(a.tobytes() == b.tobytes() for a, b in zip(t.params, params))
        t.resume()
        assert t.step(t.grads(2.0), cfg, stats=stats(0.0), what="resumed") == "step" and t.head()[0] == 3.0
    # no target: the same stats row does not stop; no stats with no target: a plain step
    t = Twin(name, seed=4)
    assert t.step(t.grads(2.0), A.Cfg(lr=1e-2), stats=stats(1.0), what="no target") == "step"
    assert t.step(t.grads(2.0), A.Cfg(lr=1e-2), what="no stats") == "step"
