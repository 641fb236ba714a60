"""macm_ppo_grad_rows and macm_adv_moments without a GPU, in the manner of test_ppo_abi.py: the library exports
them, the header and the ctypes mirror declare them, the ABI version did not move, and every refusal that is
decided before a device call answers MACM_E_INVALID with a message (the pointers are never followed):
everything macm_ppo_grad refuses, n_src out of range, index and adv_norm both NULL, misaligned index / adv_norm;
and gym_macm.ppo's ValueErrors for the new arguments."""
import ctypes

import pytest
import torch

from test_abi import declared_functions
from test_ppo_abi import cfg_of, net, refused, workspace

from gym_macm import _abi
from gym_macm import ppo

NEW = ("macm_ppo_grad_rows", "macm_adv_moments")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    rows_args, grad_args = _abi.SIGNATURES["macm_ppo_grad_rows"][1], _abi.SIGNATURES["macm_ppo_grad"][1]
    # macm_ppo_grad's arguments with index, n_src and adv_norm behind rows
    assert len(rows_args) == 20 and rows_args[:6] == grad_args[:6] and rows_args[9:] == grad_args[6:]
    assert rows_args[6:9] == [VP, ctypes.c_int64, VP]
    assert _abi.SIGNATURES["macm_adv_moments"][1] == [VP, VP, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, VP, VP,
                                                      ctypes.c_int64, VP]
    assert L.macm_abi_version() == 9


GRAD_ARGS = ("actions", "old_logp", "adv", "ret", "old_values", "grad_policy", "grad_value", "stats")


def test_ppo_grad_rows_refusals():
    f = _abi.lib().macm_ppo_grad_rows
    base = {n: VP(0x1000 * (i + 2)) for i, n in enumerate(GRAD_ARGS)}
    base["old_values"] = None
    enough = workspace(4)
    pol, crit = net(_abi.MacmPolicyMlp), net(_abi.MacmValueMlp)

    def call(cfg=cfg_of(), p=pol, c=crit, obs=VP(0x200000), rows=4, index=VP(0x300000), n_src=100, norm=VP(0x400000),
             ws=VP(0x100000), nbytes=enough, **kw):
        a = dict(base, **kw)
        return f(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(p) if p is not None else None,
                 ctypes.byref(c) if c is not None else None, obs, 0, rows, index, n_src, norm,
                 *[a[n] for n in GRAD_ARGS], ws, nbytes, None)

    # its own
    refused(call(index=None, norm=None), b"index", b"adv_norm", b"both NULL")
    for bad in (-1, 2 ** 31, 2 ** 40):
        refused(call(n_src=bad), b"n_src")
        refused(call(n_src=bad, index=None), b"n_src")
    for bad in (0x300001, 0x300002):
        refused(call(index=VP(bad)), b"index", b"aligned")
    for bad in (0x400001, 0x400004):
        refused(call(norm=VP(bad)), b"adv_norm", b"aligned")
        refused(call(norm=VP(bad), index=None), b"adv_norm", b"aligned")
    # macm_ppo_grad's, with the index alone, the normalisation alone and both
    for kw in (dict(), dict(norm=None), dict(index=None)):
        refused(call(p=None, c=None, **kw), b"both NULL")
        refused(call(cfg=None, **kw), b"cfg", b"NULL")
        refused(call(cfg=cfg_of(clip=0.0), **kw), b"clip")
        refused(call(cfg=cfg_of(ent_coef=-1.0), **kw), b"ent_coef")
        refused(call(cfg=cfg_of(vf_coef=-1.0), **kw), b"vf_coef")
        refused(call(cfg=cfg_of(vf_clip=0.0), old_values=VP(0x9000), **kw), b"vf_clip")
        refused(call(cfg=cfg_of(reserved=(0, 0, 0, 1)), **kw), b"reserved")
        refused(call(rows=-1, **kw), b"rows")
        refused(call(p=net(_abi.MacmPolicyMlp, hidden=24), **kw), b"policy", b"hidden")
        refused(call(c=net(_abi.MacmValueMlp, params=0), **kw), b"critic", b"params")
        refused(call(c=net(_abi.MacmValueMlp, in_dim=6), **kw), b"in_dim")
        refused(call(obs=None, **kw), b"obs", b"NULL")
        for n in ("actions", "old_logp", "adv", "grad_policy"):
            refused(call(**{n: None}, **kw), b"policy", b"NULL")
        for n in ("ret", "grad_value"):
            refused(call(**{n: None}, **kw), b"critic", b"NULL")
        refused(call(adv=VP(base["adv"].value + 1), **kw), b"aligned")
        refused(call(stats=VP(base["stats"].value + 4), **kw), b"stats", b"aligned")
        refused(call(ws=None, **kw), b"workspace", b"NULL")
        refused(call(ws=VP(0x100004), **kw), b"workspace", b"aligned")
        refused(call(nbytes=enough - 1, **kw), b"workspace_bytes")
        refused(call(rows=65, nbytes=workspace(64), **kw), b"workspace_bytes")


def test_adv_moments_refusals():
    f = _abi.lib().macm_adv_moments
    enough = workspace(4)

    def call(x=VP(0x1000), index=VP(0x2000), n_src=100, rows=4, eps=1e-8, out=VP(0x3000), ws=VP(0x100000),
             nbytes=enough):
        return f(x, index, n_src, rows, eps, out, ws, nbytes, None)

    refused(call(x=None), b"x", b"NULL")
    refused(call(out=None), b"out", b"NULL")
    refused(call(rows=-1), b"rows")
    for bad in (-1, 2 ** 31):
        refused(call(n_src=bad), b"n_src")
        refused(call(n_src=bad, index=None), b"n_src")
    for bad in (-1e-8, float("nan"), float("inf")):
        refused(call(eps=bad), b"eps")
    refused(call(x=VP(0x1002)), b"aligned")
    refused(call(index=VP(0x2001)), b"aligned")
    refused(call(out=VP(0x3004)), b"out", b"aligned")
    refused(call(ws=None), b"workspace", b"NULL")
    refused(call(ws=VP(0x100008)), b"workspace", b"aligned")
    refused(call(nbytes=enough - 1), b"workspace_bytes")
    refused(call(rows=65, nbytes=workspace(64)), b"workspace_bytes")


def test_python_value_errors():
    f = torch.zeros(5)
    with pytest.raises(ValueError, match="GPU device"):
        ppo.adv_moments(f)
    meta = lambda *s, **k: torch.zeros(*s, device="meta", **k)  # a device that is not the CPU, without a GPU
    with pytest.raises(ValueError, match="must be a contiguous"):
        ppo.adv_moments(meta(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="must be a contiguous"):
        ppo.adv_moments(meta(10)[::2])
    for bad in (meta(4, dtype=torch.int16), meta(2, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="index must be"):
            ppo.adv_moments(meta(5), index=bad)
    with pytest.raises(ValueError, match="eps"):
        ppo.adv_moments(meta(5), eps=-1.0)
    with pytest.raises(ValueError, match="both None"):
        ppo.ppo_grads(None, None, torch.zeros(5, 4), None, f, f, f, index=torch.zeros(2, dtype=torch.int32), adv_norm=None)
