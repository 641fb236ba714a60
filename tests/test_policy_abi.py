"""The policy entry points of include/macm.h without a GPU: the library exports them, the ctypes mirror
declares them, the ABI version did not move, macm_policy_mlp is laid out as a C compiler lays out the
header, and every refusal that needs no device answers MACM_E_INVALID with a message."""
import ctypes
import subprocess

from test_abi import HEADER, declared_functions

from gym_macm import _abi

NEW = ("macm_policy_flock", "macm_world_set_policy", "macm_world_rollout_policy", "macm_world_rollout_policy_traj")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    P = ctypes.POINTER(_abi.MacmPolicyMlp)
    assert _abi.SIGNATURES["macm_policy_flock"][1] == [P, VP, ctypes.c_int32, ctypes.c_int64, VP, VP, VP, VP]
    assert _abi.SIGNATURES["macm_world_set_policy"][1] == [VP, P]
    roll = [VP, VP, ctypes.c_int32, VP, VP, ctypes.POINTER(_abi.MacmOutputs), VP]
    assert _abi.SIGNATURES["macm_world_rollout_policy"][1] == roll
    assert _abi.SIGNATURES["macm_world_rollout_policy_traj"][1] == roll


def test_abi_version_stays_9():
    assert _abi.lib().macm_abi_version() == 9


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "macm_policy_mlp", _abi.MacmPolicyMlp
    assert [f for f, _ in cls._fields_] == ["in_dim", "hidden", "n_hidden", "reserved", "params"]
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


def policy(in_dim=4, hidden=32, n_hidden=2, reserved=0, params=0x1000):
    return _abi.MacmPolicyMlp(in_dim, hidden, n_hidden, reserved, VP(params) if params else None)


def test_null_world_is_refused():
    L = _abi.lib()
    p = policy()
    for arg in (None, ctypes.byref(p)):
        refused(L.macm_world_set_policy(None, arg), b"world", b"NULL")
    out = _abi.MacmOutputs()
    for fn in (L.macm_world_rollout_policy, L.macm_world_rollout_policy_traj):
        refused(fn(None, VP(0x1000), 3, None, None, ctypes.byref(out), None), b"world", b"NULL")
        assert fn(None, None, 0, None, None, None, None) == 0, "n_steps = 0 does nothing"
        refused(fn(None, VP(0x1000), -1, None, None, ctypes.byref(out), None), b"n_steps")


def test_policy_flock_refusals():
    """Checked before anything is launched: the pointers are never followed."""
    L = _abi.lib()
    obs, act = VP(0x2000), VP(0x3000)

    def call(p, obs=obs, act=act, rows=4):
        return L.macm_policy_flock(ctypes.byref(p) if p is not None else None, obs, 0, rows, None, act, None, None)

    refused(call(None), b"policy", b"NULL")
    refused(call(policy(params=0)), b"params", b"NULL")
    for off in (4, 8, 12, 1):
        refused(call(policy(params=0x1000 + off)), b"params", b"aligned")
    for h in (0, 8, 17, 31, 33, 64, -16):
        refused(call(policy(hidden=h)), b"hidden")
    for n in (0, 3, -1):
        refused(call(policy(n_hidden=n)), b"n_hidden")
    for d in (0, 3, 5, 7, 8):
        refused(call(policy(in_dim=d)), b"in_dim")
    for r in (1, -1):
        refused(call(policy(reserved=r)), b"reserved")
    refused(call(policy(), obs=None), b"obs")
    refused(call(policy(), act=None), b"actions")
    refused(call(policy(), rows=-1), b"rows")
