"""The PPO entry points of include/macm.h without a GPU: the library exports them, the ctypes mirror declares
them, the ABI version did not move, macm_ppo_config is laid out as a C compiler lays it out, every refusal that
is decided before a device call answers MACM_E_INVALID with a message (the pointers are never followed), the
workspace size is a nondecreasing function of rows, and gym_macm.ppo refuses what it must with ValueErrors."""
import ctypes

import pytest
import torch

from test_abi import declared_functions

from gym_macm import _abi
from gym_macm import policy as P
from gym_macm import ppo

NEW = ("macm_policy_logp", "macm_ppo_workspace", "macm_ppo_loss", "macm_ppo_grad")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    assert len(_abi.SIGNATURES["macm_policy_logp"][1]) == 6
    assert len(_abi.SIGNATURES["macm_ppo_loss"][1]) == 16
    assert len(_abi.SIGNATURES["macm_ppo_grad"][1]) == 17
    assert L.macm_abi_version() == 9


def test_config_layout():
    c = _abi.MacmPpoConfig
    assert [f for f, _ in c._fields_] == ["clip", "vf_coef", "ent_coef", "vf_clip", "reserved"]
    assert ctypes.sizeof(c) == 32 and ctypes.alignment(c) == 4
    assert [getattr(c, f).offset for f in ("clip", "vf_coef", "ent_coef", "vf_clip", "reserved")] == [0, 4, 8, 12, 16]
    cfg = ppo.config(0.2, 0.5, 0.01, 0.3)
    assert list(cfg.reserved) == [0, 0, 0, 0] and abs(cfg.vf_clip - 0.3) < 1e-7 and ppo.config().vf_clip == 0.0
    for cls in (_abi.MacmPolicyMlp, _abi.MacmValueMlp):
        assert ctypes.sizeof(cls) == 24 and cls.params.offset == 16


def refused(code, *words):
    assert code == _abi.E_INVALID, code
    msg = _abi.lib().macm_last_error()
    assert msg
    for w in words:
        assert w in msg, (w, msg)


def workspace(rows):
    n = ctypes.c_int64(-1)
    assert _abi.lib().macm_ppo_workspace(rows, ctypes.byref(n)) == 0
    return n.value


def grad_workspace(rows):
    n = ctypes.c_int64(-1)
    assert _abi.lib().macm_mlp_grad_workspace(rows, ctypes.byref(n)) == 0
    return n.value


def test_workspace_is_nondecreasing_and_covers_both_regions():
    L = _abi.lib()
    refused(L.macm_ppo_workspace(-1, ctypes.byref(ctypes.c_int64())), b"rows")
    refused(L.macm_ppo_workspace(4, None), b"bytes", b"NULL")
    tile, cap = P.GRAD_TILE_ROWS, P.GRAD_MAX_PARTIALS
    rows = [0, 1, tile - 1, tile, tile + 1, 255, 256, 257, 1000, 10 ** 4, tile * cap - 1, tile * cap, tile * cap + 1,
            256 * 2048 + 1, 10 ** 7, 2 ** 31, 2 ** 40]
    sizes = [workspace(r) for r in rows]
    assert sizes == sorted(sizes) and sizes[0] == 0
    for r in rows:  # the gradient partials, and one stat partial of 8 doubles per wave behind them
        waves = min(-(-r // tile), cap)
        assert workspace(r) >= grad_workspace(r) + waves * 64 and workspace(r) % 16 == 0
        assert workspace(r) <= grad_workspace(r) + waves * 64 + 16
    assert workspace(tile * cap) == workspace(2 ** 40)


def cfg_of(clip=0.2, vf_coef=0.5, ent_coef=0.01, vf_clip=0.0, reserved=(0, 0, 0, 0)):
    return _abi.MacmPpoConfig(clip, vf_coef, ent_coef, vf_clip, (ctypes.c_int32 * 4)(*reserved))


LOSS_ARGS = ("logits", "actions", "old_logp", "adv", "values", "ret", "old_values", "scale", "dlogits", "dvalues", "stats")


def test_ppo_loss_refusals():
    f = _abi.lib().macm_ppo_loss
    base = {n: VP(0x1000 * (i + 1)) for i, n in enumerate(LOSS_ARGS)}
    base["old_values"] = None
    enough = workspace(4)

    def call(cfg=cfg_of(), rows=4, ws=VP(0x100000), nbytes=enough, **kw):
        a = dict(base, **kw)
        return f(ctypes.byref(cfg) if cfg is not None else None, rows, *[a[n] for n in LOSS_ARGS], ws, nbytes, None)

    refused(call(cfg=None), b"cfg", b"NULL")
    for c in (0.0, -0.2, float("nan")):
        refused(call(cfg=cfg_of(clip=c)), b"clip")
    refused(call(cfg=cfg_of(vf_coef=-0.5)), b"vf_coef")
    refused(call(cfg=cfg_of(ent_coef=-0.01)), b"ent_coef")
    for v in (0.0, -0.1):
        refused(call(cfg=cfg_of(vf_clip=v), old_values=VP(0x9000)), b"vf_clip")
    for i in range(4):
        refused(call(cfg=cfg_of(reserved=[int(j == i) for j in range(4)])), b"reserved")
    refused(call(rows=-1), b"rows")
    for n in ("actions", "old_logp", "adv"):
        refused(call(**{n: None}), b"actions/old_logp/adv", b"NULL")
    refused(call(ret=None), b"ret", b"NULL")
    refused(call(logits=None, values=None, dlogits=None, dvalues=None), b"both NULL")
    refused(call(logits=None), b"dlogits")
    refused(call(values=None), b"dvalues")
    for n in ("logits", "old_logp", "adv", "values", "ret", "scale", "dlogits", "dvalues"):
        refused(call(**{n: VP(base[n].value + 2)}), b"aligned")
    refused(call(cfg=cfg_of(vf_clip=0.2), old_values=VP(0x9001)), b"aligned")
    refused(call(stats=VP(base["stats"].value + 4)), b"stats", b"aligned")
    refused(call(ws=None), b"workspace", b"NULL")
    refused(call(ws=VP(0x100008)), b"workspace", b"aligned")
    refused(call(nbytes=enough - 1), b"workspace_bytes")
    refused(call(nbytes=0), b"workspace_bytes")
    refused(call(rows=65, nbytes=workspace(64)), b"workspace_bytes")


def net(cls, in_dim=4, hidden=32, n_hidden=2, reserved=0, params=0x1000):
    return cls(in_dim, hidden, n_hidden, reserved, VP(params) if params else None)


GRAD_ARGS = ("actions", "old_logp", "adv", "ret", "old_values", "grad_policy", "grad_value", "stats")


def test_ppo_grad_refusals():
    f = _abi.lib().macm_ppo_grad
    base = {n: VP(0x1000 * (i + 2)) for i, n in enumerate(GRAD_ARGS)}
    base["old_values"] = None
    enough = workspace(4)
    pol, crit = net(_abi.MacmPolicyMlp), net(_abi.MacmValueMlp)

    def call(cfg=cfg_of(), p=pol, c=crit, obs=VP(0x200000), rows=4, ws=VP(0x100000), nbytes=enough, **kw):
        a = dict(base, **kw)
        return f(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(p) if p is not None else None,
                 ctypes.byref(c) if c is not None else None, obs, 0, rows, *[a[n] for n in GRAD_ARGS], ws, nbytes, None)

    refused(call(p=None, c=None), b"both NULL")
    refused(call(cfg=None), b"cfg", b"NULL")
    refused(call(cfg=cfg_of(clip=0.0)), b"clip")
    refused(call(cfg=cfg_of(ent_coef=-1.0)), b"ent_coef")
    refused(call(cfg=cfg_of(vf_clip=0.0), old_values=VP(0x9000)), b"vf_clip")
    refused(call(cfg=cfg_of(reserved=(0, 0, 0, 1))), b"reserved")
    refused(call(rows=-1), b"rows")
    refused(call(p=net(_abi.MacmPolicyMlp, hidden=24)), b"policy", b"hidden")
    refused(call(c=net(_abi.MacmValueMlp, params=0)), b"critic", b"params")
    refused(call(c=net(_abi.MacmValueMlp, in_dim=6)), b"in_dim")
    refused(call(obs=None), b"obs", b"NULL")
    for n in ("actions", "old_logp", "adv", "grad_policy"):
        refused(call(**{n: None}), b"policy", b"NULL")
    for n in ("ret", "grad_value"):
        refused(call(**{n: None}), b"critic", b"NULL")
    refused(call(adv=VP(base["adv"].value + 1)), b"aligned")
    refused(call(ws=None), b"workspace", b"NULL")
    refused(call(ws=VP(0x100004)), b"workspace", b"aligned")
    refused(call(nbytes=enough - 1), b"workspace_bytes")
    refused(call(rows=65, nbytes=workspace(64)), b"workspace_bytes")


def test_policy_logp_refusals():
    f = _abi.lib().macm_policy_logp
    lg, a, lp = VP(0x1000), VP(0x2000), VP(0x3000)
    refused(f(None, a, 4, lp, None, None), b"NULL")
    refused(f(lg, None, 4, lp, None, None), b"NULL")
    refused(f(lg, a, 4, None, None, None), b"NULL")
    refused(f(lg, a, -1, lp, None, None), b"rows")
    refused(f(VP(0x1002), a, 4, lp, None, None), b"aligned")
    refused(f(lg, a, 4, lp, VP(0x4001), None), b"aligned")


def test_python_value_errors():
    lg, a = torch.zeros(5, 9), torch.zeros(5, 3, dtype=torch.uint8)
    f = torch.zeros(5)
    with pytest.raises(ValueError, match="GPU device"):
        ppo.log_prob(lg, a)
    with pytest.raises(ValueError, match="GPU device"):
        ppo.ppo_loss(lg, f, a, f, f, f)
    with pytest.raises(ValueError, match="both None"):
        ppo.ppo_loss(None, None, a, f, f, f)
    with pytest.raises(ValueError, match="both None"):
        ppo.ppo_grads(None, None, lg, a, f, f, f)
    with pytest.raises(ValueError, match="clip must be > 0"):
        ppo.ppo_loss(lg, f, a, f, f, f, clip=0.0)
    with pytest.raises(ValueError, match="old_values needs vf_clip"):
        ppo.ppo_loss(lg, f, a, f, f, f, old_values=f)
    with pytest.raises(ValueError, match="vf_clip needs old_values"):
        ppo.ppo_loss(lg, f, a, f, f, f, vf_clip=0.2)
    with pytest.raises(ValueError, match="logits rows must have 9"):
        ppo.ppo_loss(torch.zeros(5, 8), f, a, f, f, f)
    meta = lambda *s, **k: torch.zeros(*s, device="meta", **k)  # a device that is not the CPU, without a GPU
    for bad in (dict(actions=meta(5, 3)), dict(actions=meta(5, 3, dtype=torch.uint8)[:4]),
                dict(old_logp=meta(5, dtype=torch.float64)), dict(adv=meta(10)[::2]), dict(ret=meta(6)),
                dict(values=meta(5, 1))):
        kw = dict(logits=meta(5, 9), values=meta(5), actions=meta(5, 3, dtype=torch.uint8), old_logp=meta(5), adv=meta(5),
                  ret=meta(5))
        kw.update(bad)
        with pytest.raises(ValueError, match="must be a contiguous"):
            ppo.ppo_loss(**kw)
