"""The set policy's gradient entry points of include/macm.h without a GPU: the library exports them, the ctypes
mirror declares them, the ABI version did not move, every refusal that is decided before a device call answers
MACM_E_INVALID with a message, the workspace size is a nondecreasing function of rows that is constant past the
cap, and forward / param_grad refuse what they must with ValueErrors."""
import ctypes

import pytest
import torch

from test_abi import declared_functions

from gym_macm import _abi
from gym_macm import policy as P
from gym_macm import tdm_policy as TP

NEW = ("macm_tdm_grad_workspace", "macm_tdm_policy_grad")
VP = ctypes.c_void_p
MAX_PARAMS = TP.n_params(32)  # the larger of the two nets


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    assert _abi.SIGNATURES["macm_tdm_grad_workspace"][1] == [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    assert _abi.SIGNATURES["macm_tdm_policy_grad"][1] == [
        ctypes.POINTER(_abi.MacmTdmPolicy), VP, VP, VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, VP, VP, VP, VP,
        ctypes.c_int64, VP]


def test_abi_version_stays_9_and_the_struct_is_untouched():
    assert _abi.lib().macm_abi_version() == 9
    assert [f for f, _ in _abi.MacmTdmPolicy._fields_] == ["hidden", "reserved", "params"]
    assert ctypes.sizeof(_abi.MacmTdmPolicy) == 24 and _abi.MacmTdmPolicy.params.offset == 16


def refused(code, *words):
    assert code == _abi.E_INVALID, code
    msg = _abi.lib().macm_last_error()
    assert msg
    for w in words:
        assert w in msg, (w, msg)


def workspace(rows):
    n = ctypes.c_int64(-1)
    assert _abi.lib().macm_tdm_grad_workspace(rows, ctypes.byref(n)) == 0
    return n.value


def test_workspace_is_monotone_and_constant_past_the_cap():
    L = _abi.lib()
    refused(L.macm_tdm_grad_workspace(-1, ctypes.byref(ctypes.c_int64())), b"rows")
    refused(L.macm_tdm_grad_workspace(4, None), b"bytes", b"NULL")
    tile, cap = P.GRAD_TILE_ROWS, P.GRAD_MAX_PARTIALS
    assert workspace(0) == 0
    at_cap = workspace(tile * cap)
    assert at_cap == cap * MAX_PARAMS * 4, "one partial of the larger net per wave"
    rows = [0, 1, tile - 1, tile, tile + 1, 1000, 10 ** 4, tile * cap - tile, tile * cap - tile + 1, tile * cap,
            tile * cap + 1, 10 ** 7, 2 ** 31, 2 ** 40]
    sizes = [workspace(r) for r in rows]
    assert sizes == sorted(sizes)
    assert workspace(1) == workspace(tile) == MAX_PARAMS * 4 and workspace(tile + 1) == 2 * MAX_PARAMS * 4
    assert workspace(tile * cap - tile) < at_cap
    for r in rows:
        if r >= tile * cap - tile + 1:
            assert workspace(r) == at_cap, r


def pol(hidden=32, reserved=(0, 0, 0), params=0x1000):
    return _abi.MacmTdmPolicy(hidden, (ctypes.c_int32 * 3)(*reserved), VP(params) if params else None)


def test_grad_refusals():
    """Checked before anything is launched: the pointers are never followed."""
    f = _abi.lib().macm_tdm_policy_grad
    ptr = dict(obs=VP(0x2000), mask=VP(0x2800), health=VP(0x3000), dlogits=VP(0x4000), grad=VP(0x5000), ws=VP(0x6000))
    enough = workspace(6)

    def call(s, n_agents=3, rows=6, nbytes=enough, agents=None, **kw):
        a = dict(ptr, **kw)
        return f(ctypes.byref(s) if s is not None else None, a["obs"], a["mask"], a["health"], 0, n_agents, rows,
                 agents, a["dlogits"], a["grad"], a["ws"], nbytes, None)

    refused(call(None), b"policy", b"NULL")
    refused(call(pol(params=0)), b"params", b"NULL")
    for off in (4, 8, 12, 1):
        refused(call(pol(params=0x1000 + off)), b"params", b"aligned")
    for h in (0, 8, 17, 31, 33, 64, -16):
        refused(call(pol(hidden=h)), b"hidden")
    for r in ((1, 0, 0), (0, -1, 0), (0, 0, 7)):
        refused(call(pol(reserved=r)), b"reserved")
    for name in ("obs", "mask", "health"):
        refused(call(pol(), **{name: None}), name.encode(), b"NULL")
    for off in (4, 8, 1):
        refused(call(pol(), obs=VP(0x2000 + off)), b"obs", b"aligned")
    refused(call(pol(), dlogits=None), b"dlogits", b"NULL")
    refused(call(pol(), grad=None), b"grad", b"NULL")
    for n in (1, 0, -3):
        refused(call(pol(), n_agents=n), b"n_agents")
    refused(call(pol(), rows=-3), b"rows")
    for r in (5, 7, 1):
        refused(call(pol(), rows=r), b"rows", b"multiple")
    refused(call(pol(), ws=None), b"workspace", b"NULL")
    for off in (4, 8, 1):
        refused(call(pol(), ws=VP(0x6000 + off)), b"workspace", b"aligned")
    refused(call(pol(), nbytes=enough - 1), b"workspace_bytes")
    refused(call(pol(), nbytes=0), b"workspace_bytes")
    refused(call(pol(), rows=66, nbytes=workspace(64)), b"workspace_bytes")
    refused(call(pol(), rows=0, obs=None, ws=None, nbytes=0), b"obs", b"NULL")  # rows = 0 excuses the workspace only
    refused(call(pol(), rows=0, grad=None, ws=None, nbytes=0), b"grad", b"NULL")


def shell(hidden=32, requires_grad=True):
    """A TdmSetPolicy without its device allocation (its constructor needs a GPU): enough of one for the checks
    that forward and param_grad make before any library call."""
    m = TP.TdmSetPolicy.__new__(TP.TdmSetPolicy)
    m.device, m.hidden, m.shapes = torch.device("cpu"), hidden, TP.layer_shapes(hidden)
    m.params = torch.zeros(TP.n_params(hidden), requires_grad=requires_grad)
    return m


def test_forward_and_param_grad_value_errors():
    E, N = 2, 3
    obs, mask = torch.zeros(E, N, N - 1, 4), torch.zeros(E, N, N - 1, dtype=torch.uint8)
    health, dl = torch.zeros(E, N, dtype=torch.float64), torch.zeros(E, N, 11)
    for rg in (True, False):
        m = shell(requires_grad=rg)
        with pytest.raises(ValueError, match="must not require grad"):
            m.forward(torch.zeros(E, N, N - 1, 4, requires_grad=True), mask, health)
        with pytest.raises(ValueError, match="obs must be a contiguous float32/float64"):
            m.forward(obs.to(torch.float16), mask, health)
        with pytest.raises(ValueError, match=r"obs must be \[\.\.\., N, N-1, 4\]"):
            m.forward(torch.zeros(E, N, N, 4), mask, health)
        with pytest.raises(ValueError, match="mask must be a contiguous uint8"):
            m.forward(obs, mask.to(torch.int32), health)
        with pytest.raises(ValueError, match="health must be a contiguous float64"):
            m.forward(obs, mask, health.to(torch.float32))
        with pytest.raises(ValueError, match="agents must be a contiguous uint8"):
            m.forward(obs, mask, health, agents=torch.zeros(N + 1, dtype=torch.uint8))
    m = shell()
    for bad in (dl.to(torch.float64), torch.zeros(E, N, 9), torch.zeros(E, N, 11, 2)[..., 0], torch.zeros(E, N, 11, device="meta")):
        with pytest.raises(ValueError, match="dlogits must be a contiguous float32"):
            m.param_grad(obs, mask, health, bad)
    with pytest.raises(ValueError, match="agents must be a contiguous uint8"):
        m.param_grad(obs, mask, health, dl, agents=torch.zeros(N, dtype=torch.int32))
