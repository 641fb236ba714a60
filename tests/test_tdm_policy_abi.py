"""The TDM policy entry points of include/macm.h without a GPU: the library exports them, the ctypes mirror
declares them, the ABI version did not move, macm_tdm_policy is laid out as a C compiler lays out the
header, and every refusal that needs no device answers MACM_E_INVALID with a message."""
import ctypes
import subprocess

from test_abi import HEADER, declared_functions

from gym_macm import _abi

NEW = ("macm_policy_tdm", "macm_tdm_set_policy", "macm_tdm_rollout_policy", "macm_tdm_rollout_policy_traj")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    P = ctypes.POINTER(_abi.MacmTdmPolicy)
    assert _abi.SIGNATURES["macm_policy_tdm"][1] == [P, VP, VP, VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, VP,
                                                     VP, VP, VP, VP]
    assert _abi.SIGNATURES["macm_tdm_set_policy"][1] == [VP, P, ctypes.c_uint32]
    roll = [VP, VP, ctypes.c_int32, VP, VP, ctypes.POINTER(_abi.MacmTdmOutputs), VP]
    assert _abi.SIGNATURES["macm_tdm_rollout_policy"][1] == roll
    assert _abi.SIGNATURES["macm_tdm_rollout_policy_traj"][1] == roll
    src = open(HEADER).read()
    assert "typedef struct macm_tdm_policy" in src, "the fifth name: the struct the entry points take"


def test_abi_version_stays_9():
    assert _abi.lib().macm_abi_version() == 9


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "macm_tdm_policy", _abi.MacmTdmPolicy
    assert [f for f, _ in cls._fields_] == ["hidden", "reserved", "params"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in cls._fields_:
        lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.split("\n") if line)
    assert int(got[cname]) == ctypes.sizeof(cls) == 24
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f


def refused(code, *words):
    assert code == _abi.E_INVALID, code
    msg = _abi.lib().macm_last_error()
    for w in words:
        assert w in msg, (w, msg)


def policy(hidden=32, reserved=(0, 0, 0), params=0x1000):
    return _abi.MacmTdmPolicy(hidden, (ctypes.c_int32 * 3)(*reserved), VP(params) if params else None)


def test_null_world_is_refused():
    L = _abi.lib()
    p = policy()
    for arg in (None, ctypes.byref(p)):
        refused(L.macm_tdm_set_policy(None, arg, 1), b"tdm", b"NULL")
    out = _abi.MacmTdmOutputs()
    for fn in (L.macm_tdm_rollout_policy, L.macm_tdm_rollout_policy_traj):
        refused(fn(None, VP(0x1000), 3, None, None, ctypes.byref(out), None), b"tdm", b"NULL")
        assert fn(None, None, 0, None, None, None, None) == 0, "n_steps = 0 does nothing"
        refused(fn(None, VP(0x1000), -1, None, None, ctypes.byref(out), None), b"n_steps")


def test_policy_tdm_refusals():
    """Checked before anything is launched: the pointers are never followed."""
    L = _abi.lib()
    obs, mask, health, act = VP(0x2000), VP(0x3000), VP(0x4000), VP(0x5000)

    def call(p, obs=obs, mask=mask, health=health, act=act, n=4, rows=8):
        return L.macm_policy_tdm(ctypes.byref(p) if p is not None else None, obs, mask, health, 0, n, rows, None, None,
                                 act, None, None)

    refused(call(None), b"policy", b"NULL")
    refused(call(policy(params=0)), b"params", b"NULL")
    for off in (4, 8, 12, 1):
        refused(call(policy(params=0x1000 + off)), b"params", b"aligned")
    for h in (0, 8, 17, 31, 33, 64, -16):
        refused(call(policy(hidden=h)), b"hidden")
    for r in ((1, 0, 0), (0, -1, 0), (0, 0, 7)):
        refused(call(policy(reserved=r)), b"reserved")
    refused(call(policy(), obs=None), b"obs")
    refused(call(policy(), mask=None), b"mask")
    refused(call(policy(), health=None), b"health")
    refused(call(policy(), act=None), b"actions")
    refused(call(policy(), obs=VP(0x2008)), b"obs", b"aligned")
    refused(call(policy(), act=VP(0x5002)), b"actions", b"aligned")
    refused(call(policy(), n=1, rows=4), b"n_agents")
    refused(call(policy(), rows=-4), b"rows")
    for rows in (7, 9, 1):
        refused(call(policy(), rows=rows), b"rows", b"multiple")
    assert call(policy(), rows=0) == 0, "no rows: nothing is launched"
