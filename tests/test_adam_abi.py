"""macm_ppo_adam, macm_ppo_update and their size calls without a GPU, in the manner of test_minibatch_abi.py: the
library exports them, the header and the ctypes mirror declare them, macm_adam_config is laid out as a C
compiler lays it out from the header, the ABI version did not move, the state and workspace sizes are what the
header says, and every refusal that is decided before a device call answers MACM_E_INVALID with a message
(the pointers are never followed); and gym_macm.ppo's ValueErrors for the new class and function."""
import ctypes
import os
import subprocess

import pytest
import torch

from test_abi import HEADER, declared_functions
from test_ppo_abi import cfg_of, net, refused, workspace

from gym_macm import _abi
from gym_macm import ppo

NEW = ("macm_ppo_adam_state_bytes", "macm_ppo_adam", "macm_ppo_update_workspace", "macm_ppo_update")
VP = ctypes.c_void_p
I32, I64, F64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
P = ctypes.POINTER


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    S = _abi.SIGNATURES
    nets = [P(_abi.MacmPolicyMlp), P(_abi.MacmValueMlp)]
    assert S["macm_ppo_adam_state_bytes"][1] == nets + [P(I64)]
    assert S["macm_ppo_adam"][1] == [P(_abi.MacmAdamConfig)] + nets + [VP, VP, VP, VP, I64, VP]
    assert S["macm_ppo_update_workspace"][1] == [I64, P(I64)]
    assert S["macm_ppo_update"][1] == ([P(_abi.MacmPpoConfig), P(_abi.MacmAdamConfig)] + nets + [VP, I32, I64] +
                                       [VP] * 5 + [I32, P(VP), P(I64), I32, F64, VP, I64, VP, VP, I64, VP])
    assert L.macm_abi_version() == 9


def test_config_layout_matches_header(tmp_path):
    c = _abi.MacmAdamConfig
    names = ["lr", "beta1", "beta2", "eps", "max_grad_norm", "target_kl", "reserved"]
    assert [f for f, _ in c._fields_] == names
    assert ctypes.sizeof(c) == 64 and ctypes.alignment(c) == 8
    assert [getattr(c, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(macm_adam_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(macm_adam_config, {f}));' for f in names]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.split() for line in out.splitlines() if line)
    assert int(got["size"]) == ctypes.sizeof(c)
    for f in names:
        assert int(got[f]) == getattr(c, f).offset, f
    assert os.path.exists(HEADER)


def adam_of(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.0, target_kl=0.0, reserved=(0, 0, 0, 0)):
    return _abi.MacmAdamConfig(lr, beta1, beta2, eps, max_grad_norm, target_kl, (I32 * 4)(*reserved))


def state_bytes(p, c):
    n = I64(-1)
    assert _abi.lib().macm_ppo_adam_state_bytes(ctypes.byref(p) if p is not None else None,
                                                ctypes.byref(c) if c is not None else None, ctypes.byref(n)) == 0
    return n.value


def update_workspace(rows):
    n = I64(-1)
    assert _abi.lib().macm_ppo_update_workspace(rows, ctypes.byref(n)) == 0
    return n.value


def test_sizes():
    L = _abi.lib()
    pol, crit = net(_abi.MacmPolicyMlp), net(_abi.MacmValueMlp)  # 4 -> 32 -> 32 -> 9 / 1: 1,513 + 1,249
    assert state_bytes(pol, crit) == 64 + 8 * (1513 + 1249)
    assert state_bytes(pol, None) == 64 + 8 * 1513 and state_bytes(None, crit) == 64 + 8 * 1249
    small = net(_abi.MacmPolicyMlp, hidden=16, n_hidden=1), net(_abi.MacmValueMlp, hidden=16, n_hidden=1)
    assert state_bytes(*small) == 64 + 8 * (233 + 97)
    big = net(_abi.MacmPolicyMlp, in_dim=6), net(_abi.MacmValueMlp, in_dim=6)
    assert state_bytes(*big) == 64 + 8 * (1577 + 1313)
    n = I64()
    refused(L.macm_ppo_adam_state_bytes(None, None, ctypes.byref(n)), b"both NULL")
    refused(L.macm_ppo_adam_state_bytes(ctypes.byref(pol), None, None), b"bytes", b"NULL")
    refused(L.macm_ppo_adam_state_bytes(ctypes.byref(net(_abi.MacmPolicyMlp, hidden=24)), None, ctypes.byref(n)), b"hidden")
    refused(L.macm_ppo_update_workspace(-1, ctypes.byref(n)), b"max_rows")
    refused(L.macm_ppo_update_workspace(4, None), b"bytes", b"NULL")
    rows = [0, 1, 64, 65, 4097, 10 ** 6, 2 ** 31]
    sizes = [update_workspace(r) for r in rows]
    assert sizes == sorted(sizes)
    for r, s in zip(rows, sizes):  # the gradient call's workspace, the moments, a stats row and both gradients
        assert s % 16 == 0 and s >= workspace(r) + 4 * 8 + 8 * 8 + 2 * 1577 * 4 and s <= workspace(r) + 12712 + 16


def test_ppo_adam_refusals():
    f = _abi.lib().macm_ppo_adam
    pol, crit = net(_abi.MacmPolicyMlp), net(_abi.MacmValueMlp)
    enough = state_bytes(pol, crit)

    def call(opt=adam_of(), p=pol, c=crit, gp=VP(0x2000), gv=VP(0x3000), stats=VP(0x4000), state=VP(0x100000),
             nbytes=enough):
        return f(ctypes.byref(opt) if opt is not None else None, ctypes.byref(p) if p is not None else None,
                 ctypes.byref(c) if c is not None else None, gp, gv, stats, state, nbytes, None)

    refused(call(opt=None), b"opt", b"NULL")
    refused(call(p=None, c=None), b"both NULL")
    refused(call(p=net(_abi.MacmPolicyMlp, hidden=24)), b"policy", b"hidden")
    refused(call(c=net(_abi.MacmValueMlp, params=0)), b"critic", b"params")
    refused(call(c=net(_abi.MacmValueMlp, reserved=1)), b"critic", b"reserved")
    for i in range(4):
        refused(call(opt=adam_of(reserved=[int(j == i) for j in range(4)])), b"reserved")
    for bad in (-1e-3, float("nan"), float("inf")):
        refused(call(opt=adam_of(lr=bad)), b"lr")
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        refused(call(opt=adam_of(beta1=bad)), b"beta")
        refused(call(opt=adam_of(beta2=bad)), b"beta")
    for bad in (0.0, -1e-8, float("nan"), float("inf")):
        refused(call(opt=adam_of(eps=bad)), b"eps")
    for bad in (-0.5, float("nan"), float("inf")):
        refused(call(opt=adam_of(max_grad_norm=bad)), b"max_grad_norm")
        refused(call(opt=adam_of(target_kl=bad)), b"target_kl")
    refused(call(opt=adam_of(target_kl=0.01), stats=None), b"target_kl", b"stats")
    refused(call(opt=adam_of(target_kl=0.01), p=None, gp=None), b"target_kl", b"policy")
    refused(call(gp=None), b"grad_policy", b"NULL")
    refused(call(gv=None), b"grad_value", b"NULL")
    refused(call(state=None), b"state", b"NULL")
    refused(call(gp=VP(0x2002)), b"aligned")
    refused(call(gv=VP(0x3001)), b"aligned")
    refused(call(stats=VP(0x4004)), b"stats", b"aligned")
    refused(call(state=VP(0x100004)), b"state", b"aligned")
    refused(call(nbytes=enough - 1), b"state_bytes")
    refused(call(nbytes=0), b"state_bytes")
    refused(call(c=None, gv=None, nbytes=state_bytes(pol, None) - 1), b"state_bytes")


ROW_ARGS = ("actions", "old_logp", "adv", "ret", "old_values")


def test_ppo_update_refusals():
    f = _abi.lib().macm_ppo_update
    pol, crit = net(_abi.MacmPolicyMlp), net(_abi.MacmValueMlp)
    base = {n: VP(0x1000 * (i + 2)) for i, n in enumerate(ROW_ARGS)}
    base["old_values"] = None
    sbytes = state_bytes(pol, crit)

    def call(cfg=cfg_of(), opt=adam_of(), p=pol, c=crit, obs=VP(0x200000), n_src=100, n_mb=2, index=(0x300000, 0x310000),
             rows=(4, 3), norm=1, adv_eps=1e-8, state=VP(0x400000), nbytes=sbytes, stats=VP(0x500000), ws=VP(0x100000),
             wbytes=None, **kw):
        a = dict(base, **kw)
        idx = (VP * max(len(index), 1))(*index) if index is not None else None
        rws = (I64 * max(len(rows), 1))(*rows) if rows is not None else None
        if wbytes is None:
            wbytes = update_workspace(max(rows, default=0) if rows is not None else 0)
        return f(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(opt) if opt is not None else None,
                 ctypes.byref(p) if p is not None else None, ctypes.byref(c) if c is not None else None, obs, 0, n_src,
                 *[a[n] for n in ROW_ARGS], n_mb, idx, rws, norm, adv_eps, state, nbytes, stats, ws, wbytes, None)

    # its own
    refused(call(n_mb=-1), b"n_minibatches")
    refused(call(index=None), b"index", b"NULL")
    refused(call(rows=None), b"rows", b"NULL")
    refused(call(rows=(4, -1)), b"rows[1]")
    refused(call(index=(0x300000, 0)), b"index[1]", b"NULL")
    refused(call(index=(0x300002, 0x310000)), b"index[0]", b"aligned")
    for bad in (-1, 2 ** 31):
        refused(call(n_src=bad), b"n_src")
    for bad in (-1e-8, float("nan"), float("inf")):
        refused(call(adv_eps=bad), b"adv_eps")
    refused(call(ws=None), b"workspace", b"NULL")
    refused(call(ws=VP(0x100008)), b"workspace", b"aligned")
    refused(call(wbytes=update_workspace(4) - 1), b"workspace_bytes")
    refused(call(rows=(4, 65), wbytes=update_workspace(64)), b"workspace_bytes")
    # macm_ppo_grad_rows's
    refused(call(p=None, c=None), b"both NULL")
    refused(call(cfg=None), b"cfg", b"NULL")
    refused(call(cfg=cfg_of(clip=0.0)), b"clip")
    refused(call(cfg=cfg_of(ent_coef=-1.0)), b"ent_coef")
    refused(call(cfg=cfg_of(vf_coef=-1.0)), b"vf_coef")
    refused(call(cfg=cfg_of(vf_clip=0.0), old_values=VP(0x9000)), b"vf_clip")
    refused(call(cfg=cfg_of(reserved=(0, 0, 0, 1))), b"reserved")
    refused(call(p=net(_abi.MacmPolicyMlp, hidden=24)), b"policy", b"hidden")
    refused(call(c=net(_abi.MacmValueMlp, params=0)), b"critic", b"params")
    refused(call(c=net(_abi.MacmValueMlp, in_dim=6)), b"in_dim")
    refused(call(obs=None), b"obs", b"NULL")
    for n in ("actions", "old_logp", "adv"):
        refused(call(**{n: None}), b"policy", b"NULL")
    refused(call(ret=None), b"critic", b"NULL")
    refused(call(adv=VP(base["adv"].value + 1)), b"aligned")
    refused(call(stats=VP(0x500004)), b"stats", b"aligned")
    # macm_ppo_adam's
    refused(call(opt=None), b"opt", b"NULL")
    refused(call(opt=adam_of(lr=-1.0)), b"lr")
    refused(call(opt=adam_of(beta1=1.0)), b"beta")
    refused(call(opt=adam_of(eps=0.0)), b"eps")
    refused(call(opt=adam_of(max_grad_norm=-1.0)), b"max_grad_norm")
    refused(call(opt=adam_of(target_kl=float("nan"))), b"target_kl")
    refused(call(opt=adam_of(target_kl=0.01), p=None), b"target_kl", b"policy")
    refused(call(opt=adam_of(reserved=(1, 0, 0, 0))), b"reserved")
    refused(call(state=None), b"state", b"NULL")
    refused(call(state=VP(0x400004)), b"state", b"aligned")
    refused(call(nbytes=sbytes - 1), b"state_bytes")


def test_python_value_errors():
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(lr=float("nan")), "lr"), (dict(betas=(1.0, 0.999)), "betas"),
                     (dict(betas=(0.9,)), "betas"), (dict(eps=0.0), "eps"), (dict(max_grad_norm=-1.0), "max_grad_norm"),
                     (dict(target_kl=-0.01), "target_kl"), (dict(), "both None")):
        with pytest.raises(ValueError, match=word):
            ppo.Adam(None, None, **kw)
    with pytest.raises(ValueError, match="target_kl needs the policy"):
        ppo.Adam(None, object(), target_kl=0.01)
    f = torch.zeros(5)
    with pytest.raises(ValueError, match="gym_macm.ppo.Adam"):
        ppo.update(None, torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.uint8), f, f, f)
    assert ppo.ADAM_HEAD[:4] == ("t", "beta1_pow", "beta2_pow", "stopped") and len(ppo.ADAM_HEAD) == 8
