"""The critic and GAE entry points of include/macm.h without a GPU: the library exports them, the ctypes
mirror declares them, the ABI version did not move, macm_value_mlp is laid out as a C compiler lays out
the header, every refusal that is decided before a device call answers MACM_E_INVALID with a message,
and MlpCritic and gae refuse what they must with ValueErrors."""
import ctypes
import subprocess

import pytest
import torch

from test_abi import HEADER, declared_functions

from gym_macm import _abi
from gym_macm.policy import MlpCritic, MlpPolicy, gae

NEW = ("macm_value_flock", "macm_world_set_critic", "macm_world_rollout_policy_value",
       "macm_world_rollout_policy_value_traj", "macm_gae")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    P = ctypes.POINTER(_abi.MacmValueMlp)
    assert _abi.SIGNATURES["macm_value_flock"][1] == [P, VP, ctypes.c_int32, ctypes.c_int64, VP, VP]
    assert _abi.SIGNATURES["macm_world_set_critic"][1] == [VP, P]
    roll = [VP, VP, ctypes.c_int32, VP, VP, VP, VP, ctypes.POINTER(_abi.MacmOutputs), VP]
    assert _abi.SIGNATURES["macm_world_rollout_policy_value"][1] == roll
    assert _abi.SIGNATURES["macm_world_rollout_policy_value_traj"][1] == roll
    assert _abi.SIGNATURES["macm_gae"][1] == [VP, VP, VP, VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_float, ctypes.c_float, VP, VP, VP]


def test_abi_version_stays_9_and_the_policy_struct_is_untouched():
    assert _abi.lib().macm_abi_version() == 9
    assert [f for f, _ in _abi.MacmPolicyMlp._fields_] == ["in_dim", "hidden", "n_hidden", "reserved", "params"]


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "macm_value_mlp", _abi.MacmValueMlp
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


def critic(in_dim=4, hidden=32, n_hidden=2, reserved=0, params=0x1000):
    return _abi.MacmValueMlp(in_dim, hidden, n_hidden, reserved, VP(params) if params else None)


def test_null_world_is_refused():
    L = _abi.lib()
    c = critic()
    for arg in (None, ctypes.byref(c)):
        refused(L.macm_world_set_critic(None, arg), b"world", b"NULL")
    out = _abi.MacmOutputs()
    for fn in (L.macm_world_rollout_policy_value, L.macm_world_rollout_policy_value_traj):
        refused(fn(None, VP(0x1000), 3, None, None, VP(0x2000), VP(0x3000), ctypes.byref(out), None), b"world", b"NULL")
        assert fn(None, None, 0, None, None, None, None, None, None) == 0, "n_steps = 0 does nothing"
        refused(fn(None, VP(0x1000), -1, None, None, VP(0x2000), None, ctypes.byref(out), None), b"n_steps")


def test_value_flock_refusals():
    """Checked before anything is launched: the pointers are never followed."""
    L = _abi.lib()
    obs, val = VP(0x2000), VP(0x3000)

    def call(c, obs=obs, val=val, rows=4):
        return L.macm_value_flock(ctypes.byref(c) if c is not None else None, obs, 0, rows, val, None)

    refused(call(None), b"critic", b"NULL")
    refused(call(critic(params=0)), b"params", b"NULL")
    for off in (4, 8, 12, 1):
        refused(call(critic(params=0x1000 + off)), b"params", b"aligned")
    for h in (0, 8, 17, 31, 33, 64, -16):
        refused(call(critic(hidden=h)), b"hidden")
    for n in (0, 3, -1):
        refused(call(critic(n_hidden=n)), b"n_hidden")
    for d in (0, 3, 5, 7, 8):
        refused(call(critic(in_dim=d)), b"in_dim")
    for r in (1, -1):
        refused(call(critic(reserved=r)), b"reserved")
    refused(call(critic(), obs=None), b"obs")
    refused(call(critic(), val=None), b"values")
    refused(call(critic(), rows=-1), b"rows")


def test_gae_refusals():
    L = _abi.lib()
    ptrs = [VP(0x1000 * (i + 1)) for i in range(6)]  # reward, values, boot, done, adv, ret: never followed

    def call(p=ptrs, K=3, E=2, N=5):
        return L.macm_gae(p[0], p[1], p[2], p[3], K, E, N, 0.99, 0.95, p[4], p[5], None)

    for i in range(6):
        refused(call(p=[None if j == i else q for j, q in enumerate(ptrs)]), b"gae", b"NULL")
    refused(call(K=-1), b"gae", b">= 0")
    refused(call(E=-1), b"gae", b">= 0")
    refused(call(N=-2), b"gae", b">= 0")
    # nothing to do: no launch, so no device is needed and the pointers are never followed
    assert call(K=0) == 0 and call(E=0) == 0 and call(N=0) == 0


def test_mlp_critic_shape_checks():
    for bad in ((5, 32, 2), (4, 8, 2), (4, 32, 3), (6, 64, 1), (4, 32, 0)):
        with pytest.raises(ValueError, match="MlpCritic"):
            MlpCritic(*bad, device="cuda:0")
    with pytest.raises(ValueError, match="critic's params live on a GPU"):
        MlpCritic(4, 32, 2, device="cpu")
    with pytest.raises(ValueError, match="policy's params live on a GPU"):  # MlpPolicy's message is its own still
        MlpPolicy(4, 32, 2, device="cpu")
    with pytest.raises(ValueError, match="MlpPolicy"):
        MlpPolicy(5, 32, 2, device="cuda:0")
    lin = torch.nn.Linear
    with pytest.raises(ValueError, match="head with 1 output"):
        MlpCritic.from_linear_layers([lin(4, 32), lin(32, 32), lin(32, 9)], device="cpu")
    with pytest.raises(ValueError, match="head with 1 output"):
        MlpCritic.from_linear_layers([lin(4, 32)], device="cpu")
    with pytest.raises(ValueError, match="head with 9 outputs"):
        MlpPolicy.from_linear_layers([lin(4, 32), lin(32, 1)], device="cpu")
    with pytest.raises(ValueError, match="GPU"):  # the shapes pass; only the device is refused
        MlpCritic.from_linear_layers([lin(4, 32), lin(32, 32), lin(32, 1)], device="cpu")


def test_gae_value_errors():
    K, E, N = 3, 2, 4
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    rew, val, boot, done = f(K, E, N), f(K, E, N), f(K, E, N), torch.zeros((K, E), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\[K, E, N\]"):
        gae(f(K, E), val, boot, done, 0.99, 0.95)
    with pytest.raises(ValueError, match="values"):
        gae(rew, f(K + 1, E, N), boot, done, 0.99, 0.95)
    with pytest.raises(ValueError, match="values"):
        gae(rew, f(K, E, N + 1)[:, :, :N], boot, done, 0.99, 0.95)  # not contiguous
    with pytest.raises(ValueError, match="boot"):
        gae(rew, val, boot.double(), done, 0.99, 0.95)
    with pytest.raises(ValueError, match="done"):
        gae(rew, val, boot, done.bool(), 0.99, 0.95)
    with pytest.raises(ValueError, match="done"):
        gae(rew, val, boot, torch.zeros((K, E, N), dtype=torch.uint8), 0.99, 0.95)
    with pytest.raises(ValueError, match="adv"):
        gae(rew, val, boot, done, 0.99, 0.95, adv=f(K, E))
    with pytest.raises(ValueError, match="ret"):
        gae(rew, val, boot, done, 0.99, 0.95, ret=f(K, E, N).half())
    with pytest.raises(ValueError, match="alias"):
        gae(rew, val, boot, done, 0.99, 0.95, adv=rew)
    with pytest.raises(ValueError, match="alias"):
        gae(rew, val, boot, done, 0.99, 0.95, ret=val)
    both = f(K, E, N)
    with pytest.raises(ValueError, match="alias"):
        gae(rew, val, boot, done, 0.99, 0.95, adv=both, ret=both)
    with pytest.raises(ValueError, match="GPU"):  # everything else in order: CPU tensors are refused, not computed
        gae(rew, val, boot, done, 0.99, 0.95)
