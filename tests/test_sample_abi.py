"""The sampling entry points of include/macm.h without a GPU: the library exports them, the ctypes mirror
declares them, the ABI version did not move, macm_sample_config is laid out as a C compiler lays out the
header, and every refusal that needs no device answers MACM_E_INVALID with a message, those of first_row among
them. (The refusals that need a world, a continuous one and noise given while sampling is on, are in
test_gpu_rollout_sample.py; first_row against a world's rows in test_gpu_rollout_shards.py.)"""
import ctypes
import subprocess

import pytest
from test_abi import HEADER, declared_functions
from test_policy_abi import policy, refused

from gym_macm import _abi
from gym_macm.policy import sample_config

NEW = ("macm_policy_noise", "macm_policy_flock_sampled", "macm_world_set_sampling", "macm_world_get_sampling",
       "macm_policy_noise_at", "macm_policy_flock_sampled_at", "macm_world_set_sampling_at", "macm_world_get_sampling_row")
VP = ctypes.c_void_p


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        assert _abi.SIGNATURES[name][0] is ctypes.c_int
    S, P = ctypes.POINTER(_abi.MacmSampleConfig), ctypes.POINTER(_abi.MacmPolicyMlp)
    assert _abi.SIGNATURES["macm_policy_noise"][1] == [S, ctypes.c_int64, ctypes.c_int64, VP, VP, VP]
    assert _abi.SIGNATURES["macm_policy_flock_sampled"][1] == [P, VP, ctypes.c_int32, ctypes.c_int64, S, VP, VP, VP]
    assert _abi.SIGNATURES["macm_world_set_sampling"][1] == [VP, S]
    assert _abi.SIGNATURES["macm_world_get_sampling"][1] == [VP, S]
    # the _at forms: first_row, an int64, before the rows it offsets (after cfg for a world)
    I64 = ctypes.c_int64
    assert _abi.SIGNATURES["macm_policy_noise_at"][1] == [S, I64, I64, I64, VP, VP, VP]
    assert _abi.SIGNATURES["macm_policy_flock_sampled_at"][1] == [P, VP, ctypes.c_int32, I64, I64, S, VP, VP, VP]
    assert _abi.SIGNATURES["macm_world_set_sampling_at"][1] == [VP, S, I64]
    assert _abi.SIGNATURES["macm_world_get_sampling_row"][1] == [VP, ctypes.POINTER(I64)]


def test_abi_version_stays_9():
    assert _abi.lib().macm_abi_version() == 9


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "macm_sample_config", _abi.MacmSampleConfig
    assert [f for f, _ in cls._fields_] == ["seed", "decision", "reserved"]
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
    assert int(got[cname]) == ctypes.sizeof(cls) == 32
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert cls.seed.offset == 0 and cls.decision.offset == 8 and cls.reserved.offset == 16


def cfg(seed=7, decision=0, reserved=(0, 0, 0, 0)):
    return _abi.MacmSampleConfig(seed, decision, (ctypes.c_int32 * 4)(*reserved))


def test_sample_config_from_python_ints():
    c = sample_config(2**64 - 1, 2**63 + 5)
    assert c.seed == 2**64 - 1 and c.decision == 2**63 + 5 and list(c.reserved) == [0, 0, 0, 0]
    for seed, dec in ((-1, 0), (2**64, 0), (0, -1), (0, 2**64)):
        with pytest.raises(ValueError, match="2\\*\\*64"):
            sample_config(seed, dec)


def test_null_world_is_refused():
    L = _abi.lib()
    c = cfg()
    for arg in (None, ctypes.byref(c)):
        refused(L.macm_world_set_sampling(None, arg), b"world", b"NULL")
    refused(L.macm_world_get_sampling(None, ctypes.byref(c)), b"NULL")
    for arg in (None, ctypes.byref(c)):
        for first_row in (0, 64):
            refused(L.macm_world_set_sampling_at(None, arg, first_row), b"world", b"NULL")
    row = ctypes.c_int64(77)
    refused(L.macm_world_get_sampling_row(None, ctypes.byref(row)), b"NULL")
    refused(L.macm_world_get_sampling_row(None, None), b"NULL")
    assert row.value == 77


def test_policy_noise_refusals():
    """Checked before anything is launched: the pointers are never followed."""
    L = _abi.lib()
    noise = VP(0x2000)

    def call(c, n_dec=2, rows=4, noise=noise, words=None):
        return L.macm_policy_noise(ctypes.byref(c) if c is not None else None, n_dec, rows, noise, words, None)

    refused(call(None), b"cfg", b"NULL")
    for i in range(4):
        for v in (1, -1):
            r = [0, 0, 0, 0]
            r[i] = v
            refused(call(cfg(reserved=r)), b"reserved")
    refused(call(cfg(), n_dec=-1), b"n_dec")
    refused(call(cfg(), rows=-1), b"rows")
    refused(call(cfg(), rows=2**32 + 1), b"rows", b"2^32")
    refused(call(cfg(), noise=None), b"noise", b"NULL")
    refused(call(cfg(), noise=None, words=VP(0x3000)), b"noise", b"NULL")
    # nothing to write: no launch, no device needed
    assert call(cfg(), n_dec=0) == 0 and call(cfg(), rows=0) == 0


def test_policy_flock_sampled_refusals():
    L = _abi.lib()
    obs, act = VP(0x2000), VP(0x3000)

    def call(p, c, obs=obs, act=act, rows=4):
        return L.macm_policy_flock_sampled(ctypes.byref(p) if p is not None else None, obs, 0, rows,
                                           ctypes.byref(c) if c is not None else None, act, None, None)

    refused(call(None, cfg()), b"policy", b"NULL")
    refused(call(policy(params=0), cfg()), b"params", b"NULL")
    refused(call(policy(params=0x1004), cfg()), b"params", b"aligned")
    refused(call(policy(hidden=8), cfg()), b"hidden")
    refused(call(policy(n_hidden=3), cfg()), b"n_hidden")
    refused(call(policy(in_dim=5), cfg()), b"in_dim")
    refused(call(policy(reserved=1), cfg()), b"reserved")
    refused(call(policy(), None), b"cfg", b"NULL")
    refused(call(policy(), cfg(reserved=(0, 0, 0, 1))), b"sampling", b"reserved")
    refused(call(policy(), cfg(), obs=None), b"obs")
    refused(call(policy(), cfg(), act=None), b"actions")
    refused(call(policy(), cfg(), rows=-1), b"rows")
    refused(call(policy(), cfg(), rows=2**32 + 1), b"rows", b"2^32")
    assert call(policy(), cfg(), rows=0) == 0


def reserved_words():
    for i in range(4):
        for v in (1, -1):
            r = [0, 0, 0, 0]
            r[i] = v
            yield r


def test_policy_noise_at_refusals():
    """macm_policy_noise_at: macm_policy_noise's refusals at a first_row, and first_row's own. The pointers are
    never followed."""
    L = _abi.lib()
    noise = VP(0x2000)

    def call(c, first_row=64, n_dec=2, rows=4, noise=noise, words=None):
        return L.macm_policy_noise_at(ctypes.byref(c) if c is not None else None, first_row, n_dec, rows, noise, words, None)

    refused(call(None), b"cfg", b"NULL")
    for r in reserved_words():
        refused(call(cfg(reserved=r)), b"reserved")
    refused(call(cfg(), n_dec=-1), b"n_dec")
    refused(call(cfg(), rows=-1), b"rows")
    refused(call(cfg(), first_row=0, rows=2**32 + 1), b"rows", b"2^32")
    refused(call(cfg(), noise=None), b"noise", b"NULL")
    refused(call(cfg(), noise=None, words=VP(0x3000)), b"noise", b"NULL")
    refused(call(cfg(), first_row=-1), b"first_row")
    refused(call(cfg(), first_row=-2**63), b"first_row")
    for first_row, rows in ((2**32 - 3, 4), (1, 2**32), (2**32, 1), (2**32 + 1, 0), (2**63 - 1, 2**32)):
        refused(call(cfg(), first_row=first_row, rows=rows), b"first_row", b"2^32")
    # first_row + rows = 2**32 exactly is accepted; with no rows nothing is launched and no device is needed
    assert call(cfg(), first_row=2**32, rows=0) == 0
    assert call(cfg(), first_row=64, rows=0) == 0 and call(cfg(), first_row=64, n_dec=0) == 0


def test_policy_flock_sampled_at_refusals():
    L = _abi.lib()
    obs, act = VP(0x2000), VP(0x3000)

    def call(p, c, first_row=64, obs=obs, act=act, rows=4):
        return L.macm_policy_flock_sampled_at(ctypes.byref(p) if p is not None else None, obs, 0, first_row, rows,
                                              ctypes.byref(c) if c is not None else None, act, None, None)

    refused(call(None, cfg()), b"policy", b"NULL")
    refused(call(policy(params=0), cfg()), b"params", b"NULL")
    refused(call(policy(params=0x1004), cfg()), b"params", b"aligned")
    refused(call(policy(hidden=8), cfg()), b"hidden")
    refused(call(policy(n_hidden=3), cfg()), b"n_hidden")
    refused(call(policy(in_dim=5), cfg()), b"in_dim")
    refused(call(policy(reserved=1), cfg()), b"reserved")
    refused(call(policy(), None), b"cfg", b"NULL")
    for r in reserved_words():
        refused(call(policy(), cfg(reserved=r)), b"sampling", b"reserved")
    refused(call(policy(), cfg(), obs=None), b"obs")
    refused(call(policy(), cfg(), act=None), b"actions")
    refused(call(policy(), cfg(), rows=-1), b"rows")
    refused(call(policy(), cfg(), first_row=0, rows=2**32 + 1), b"rows", b"2^32")
    refused(call(policy(), cfg(), first_row=-1), b"first_row")
    for first_row, rows in ((2**32 - 3, 4), (1, 2**32), (2**32, 1), (2**32 + 1, 0)):
        refused(call(policy(), cfg(), first_row=first_row, rows=rows), b"first_row", b"2^32")
    assert call(policy(), cfg(), first_row=2**32, rows=0) == 0 and call(policy(), cfg(), rows=0) == 0


def test_first_row_from_python_ints():
    """ctypes would truncate an int past int64 silently: the Python layer refuses it first."""
    from gym_macm.policy import sample_first_row
    assert sample_first_row(0) == 0 and sample_first_row(2**32) == 2**32
    for bad in (-1, 2**32 + 1, 2**64, 2**64 + 5):
        with pytest.raises(ValueError, match="first_row"):
            sample_first_row(bad)
