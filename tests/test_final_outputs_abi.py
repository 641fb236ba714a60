"""macm_world_set_final_outputs / macm_tdm_set_final_outputs (include/macm.h) without a GPU: the
library exports them, the ctypes mirror declares them, the ABI version did not move, a NULL world is
refused with a message, and macm_final_outputs is laid out as a C compiler lays out the header."""
import ctypes
import subprocess

from test_abi import HEADER, declared_functions

from gym_macm import _abi

NEW = ("macm_world_set_final_outputs", "macm_tdm_set_final_outputs")


def test_exported_and_declared():
    L = _abi.lib()
    fns = declared_functions()
    for name in NEW:
        assert name in fns, f"{name} not declared in include/macm.h"
        assert name in _abi.SIGNATURES, f"{name} not in _abi.SIGNATURES"
        assert hasattr(L, name), f"{name} not exported"
        res, args = _abi.SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_abi.MacmFinalOutputs)]


def test_abi_version_stays_9():
    assert _abi.lib().macm_abi_version() == 9


def test_null_world_is_refused_with_a_message():
    L = _abi.lib()
    fin = _abi.MacmFinalOutputs()
    for name, word in zip(NEW, (b"world", b"tdm")):
        for arg in (None, ctypes.byref(fin)):
            assert getattr(L, name)(None, arg) == -1, name
            msg = L.macm_last_error()
            assert word in msg and b"NULL" in msg, (name, msg)


def test_struct_layout_matches_header(tmp_path):
    """As test_abi.py::test_struct_layouts_match_header, for macm_final_outputs."""
    cname, cls = "macm_final_outputs", _abi.MacmFinalOutputs
    assert [f for f, _ in cls._fields_] == ["obs", "nbr_id", "mask", "length", "ends"]
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
    assert int(got[cname]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
