"""The gradient entry points of include/macm.h without a GPU: the library exports them, the ctypes mirror
declares them, the ABI version did not move and the existing structs kept their layouts, every refusal that is
decided before a device call answers MACM_E_INVALID with a message, the workspace size is a nondecreasing
function of rows that is constant past the cap, and forward / param_grad refuse what they must with
ValueErrors."""
import ctypes

import pytest
import torch

from test_abi import declared_functions

from gym_macm import _abi
from gym_macm import policy as P

NEW = ("macm_mlp_grad_workspace", "macm_policy_grad", "macm_value_grad")
VP = ctypes.c_void_p
MAX_PARAMS = P.n_params(6, 32, 2, 9)  # the largest supported net


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    assert _abi.SIGNATURES["macm_mlp_grad_workspace"][1] == [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    tail = [VP, ctypes.c_int32, ctypes.c_int64, VP, VP, VP, ctypes.c_int64, VP]
    assert _abi.SIGNATURES["macm_policy_grad"][1] == [ctypes.POINTER(_abi.MacmPolicyMlp)] + tail
    assert _abi.SIGNATURES["macm_value_grad"][1] == [ctypes.POINTER(_abi.MacmValueMlp)] + tail


def test_abi_version_stays_9_and_the_structs_are_untouched():
    assert _abi.lib().macm_abi_version() == 9
    for cls in (_abi.MacmPolicyMlp, _abi.MacmValueMlp):
        assert [f for f, _ in cls._fields_] == ["in_dim", "hidden", "n_hidden", "reserved", "params"]
        assert ctypes.sizeof(cls) == 24 and cls.params.offset == 16
    assert [f for f, _ in _abi.MacmOutputs._fields_] == ["obs", "nbr_id", "reward", "collided", "done"]


def refused(code, *words):
    assert code == _abi.E_INVALID, code
    msg = _abi.lib().macm_last_error()
    assert msg
    for w in words:
        assert w in msg, (w, msg)


def workspace(rows):
    n = ctypes.c_int64(-1)
    assert _abi.lib().macm_mlp_grad_workspace(rows, ctypes.byref(n)) == 0
    return n.value


def test_workspace_is_monotone_and_constant_past_the_cap():
    L = _abi.lib()
    refused(L.macm_mlp_grad_workspace(-1, ctypes.byref(ctypes.c_int64())), b"rows")
    refused(L.macm_mlp_grad_workspace(4, None), b"bytes", b"NULL")
    tile, cap = P.GRAD_TILE_ROWS, P.GRAD_MAX_PARTIALS
    assert workspace(0) == 0
    at_cap = workspace(tile * cap)
    assert at_cap == cap * MAX_PARAMS * 4, "one partial of the largest net per wave"
    rows = [0, 1, tile - 1, tile, tile + 1, 1000, 10 ** 4, tile * cap - tile, tile * cap - tile + 1, tile * cap,
            tile * cap + 1, 10 ** 7, 2 ** 31, 2 ** 40]
    sizes = [workspace(r) for r in rows]
    assert sizes == sorted(sizes)
    assert workspace(1) == workspace(tile) == MAX_PARAMS * 4 and workspace(tile + 1) == 2 * MAX_PARAMS * 4
    assert workspace(tile * cap - tile) < at_cap
    for r in rows:
        if r >= tile * cap - tile + 1:
            assert workspace(r) == at_cap, r


def net(cls, in_dim=4, hidden=32, n_hidden=2, reserved=0, params=0x1000):
    return cls(in_dim, hidden, n_hidden, reserved, VP(params) if params else None)


@pytest.mark.parametrize("fn,cls,what", [("macm_policy_grad", _abi.MacmPolicyMlp, b"policy"),
                                         ("macm_value_grad", _abi.MacmValueMlp, b"critic")])
def test_grad_refusals(fn, cls, what):
    """Checked before anything is launched: the pointers are never followed."""
    L = _abi.lib()
    f = getattr(L, fn)
    obs, dout, grad, ws = VP(0x2000), VP(0x3000), VP(0x4000), VP(0x5000)
    enough = workspace(4)

    def call(s, obs=obs, dout=dout, grad=grad, ws=ws, nbytes=enough, rows=4):
        return f(ctypes.byref(s) if s is not None else None, obs, 0, rows, dout, grad, ws, nbytes, None)

    refused(call(None), what, b"NULL")
    refused(call(net(cls, params=0)), b"params", b"NULL")
    for off in (4, 8, 12, 1):
        refused(call(net(cls, params=0x1000 + off)), b"params", b"aligned")
    for h in (0, 8, 17, 31, 33, 64, -16):
        refused(call(net(cls, hidden=h)), b"hidden")
    for n in (0, 3, -1):
        refused(call(net(cls, n_hidden=n)), b"n_hidden")
    for d in (0, 3, 5, 7, 8):
        refused(call(net(cls, in_dim=d)), b"in_dim")
    for r in (1, -1):
        refused(call(net(cls, reserved=r)), b"reserved")
    refused(call(net(cls), obs=None), b"obs", b"NULL")
    refused(call(net(cls), dout=None), b"dout", b"NULL")
    refused(call(net(cls), grad=None), b"grad", b"NULL")
    refused(call(net(cls), rows=-1), b"rows")
    refused(call(net(cls), ws=None), b"workspace", b"NULL")
    for off in (4, 8, 1):
        refused(call(net(cls), ws=VP(0x5000 + off)), b"workspace", b"aligned")
    refused(call(net(cls), nbytes=enough - 1), b"workspace_bytes")
    refused(call(net(cls), nbytes=0), b"workspace_bytes")
    refused(call(net(cls), rows=65, nbytes=workspace(64)), b"workspace_bytes")
    refused(call(net(cls), rows=0, obs=None, ws=None, nbytes=0), b"obs", b"NULL")  # rows = 0 excuses the workspace only


def shell(cls, in_dim=4, hidden=32, n_hidden=2, requires_grad=True):
    """An MlpPolicy / MlpCritic without its device allocation (its constructor needs a GPU): enough of one for
    the checks that forward and param_grad make before any library call."""
    m = cls.__new__(cls)
    m.device = torch.device("cpu")
    m.in_dim, m.hidden, m.n_hidden = in_dim, hidden, n_hidden
    m.params = torch.zeros(P.n_params(in_dim, hidden, n_hidden, cls.N_OUT), requires_grad=requires_grad)
    return m


@pytest.mark.parametrize("cls,what", [(P.MlpPolicy, "policy"), (P.MlpCritic, "critic")])
def test_forward_value_errors(cls, what):
    for rg in (True, False):
        m = shell(cls, requires_grad=rg)
        with pytest.raises(ValueError, match="obs must not require grad"):
            m.forward(torch.zeros(5, 4, requires_grad=True))
        with pytest.raises(ValueError, match=f"contiguous float32/float64 tensor on the {what}'s device"):
            m.forward(torch.zeros(5, 4, dtype=torch.float16))
        with pytest.raises(ValueError, match=f"contiguous float32/float64 tensor on the {what}'s device"):
            m.forward(torch.zeros(5, 8)[:, ::2])
        with pytest.raises(ValueError, match=f"contiguous float32/float64 tensor on the {what}'s device"):
            m.forward(torch.zeros(5, 4, device="meta"))
        with pytest.raises(ValueError, match="obs rows must have 4 values"):
            m.forward(torch.zeros(5, 6))
    m = shell(cls)
    obs = torch.zeros(5, 4)
    good = (5, 9) if cls is P.MlpPolicy else (5,)
    for bad in (torch.zeros(good, dtype=torch.float64), torch.zeros((6,) + good[1:]), torch.zeros(good + (2,))[..., 0],
                torch.zeros(good, device="meta")):
        with pytest.raises(ValueError, match="dout must be a contiguous float32"):
            m.param_grad(obs, bad)
    with pytest.raises(ValueError, match="obs must not require grad"):
        m.param_grad(torch.zeros(5, 4, requires_grad=True), torch.zeros(good))
