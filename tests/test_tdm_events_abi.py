"""macm_tdm_set_events (include/macm.h) without a GPU, as test_final_outputs_abi.py: the library
exports it, the ctypes mirror declares it, the ABI version did not move, a NULL world, a misaligned
pointer and rows < 1 are refused with a message, and macm_tdm_events is laid out as a C compiler lays
out the header."""
import ctypes
import subprocess

from test_abi import HEADER, declared_functions

from gym_macm import _abi

NAME = "macm_tdm_set_events"


def test_exported_and_declared():
    L = _abi.lib()
    assert NAME in declared_functions(), f"{NAME} not declared in include/macm.h"
    assert NAME in _abi.SIGNATURES, f"{NAME} not in _abi.SIGNATURES"
    assert hasattr(L, NAME), f"{NAME} not exported"
    res, args = _abi.SIGNATURES[NAME]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_abi.MacmTdmEvents)]


def test_abi_version_stays_9():
    assert _abi.lib().macm_abi_version() == 9


def test_null_world_is_refused_with_a_message():
    L = _abi.lib()
    buf = (ctypes.c_int32 * 4)()
    ev = _abi.MacmTdmEvents(ctypes.addressof(buf), 1)
    for arg in (None, ctypes.byref(ev)):
        assert L.macm_tdm_set_events(None, arg) == -1
        msg = L.macm_last_error()
        assert b"tdm" in msg and b"NULL" in msg, msg


def test_bad_registrations_are_refused_with_a_message():
    """The registration is checked before the world is looked at, so each refusal shows its own
    message without a GPU to create a world on."""
    L = _abi.lib()
    buf = (ctypes.c_int32 * 4)()
    for off in (1, 2, 3):
        ev = _abi.MacmTdmEvents(ctypes.addressof(buf) + off, 1)
        assert L.macm_tdm_set_events(None, ctypes.byref(ev)) == -1
        assert b"aligned" in L.macm_last_error(), L.macm_last_error()
    for rows in (0, -1):
        ev = _abi.MacmTdmEvents(ctypes.addressof(buf), rows)
        assert L.macm_tdm_set_events(None, ctypes.byref(ev)) == -1
        assert b"rows" in L.macm_last_error(), L.macm_last_error()
    # rows is not looked at when the registration is being cleared
    assert L.macm_tdm_set_events(None, ctypes.byref(_abi.MacmTdmEvents(None, 0))) == -1
    assert b"NULL" in L.macm_last_error()


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "macm_tdm_events", _abi.MacmTdmEvents
    assert [f for f, _ in cls._fields_] == ["hit_id", "rows"]
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
