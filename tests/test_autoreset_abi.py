"""macm_world_set_autoreset / macm_tdm_set_autoreset without a GPU: the library exports both, and a
NULL world is refused with a message (no abort). The additive change leaves MACM_ABI_VERSION at 9
(tests/test_abi.py pins it and checks the header against the ctypes mirror)."""
import pytest

from gym_macm import _abi

NAMES = ("macm_world_set_autoreset", "macm_tdm_set_autoreset")


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_set_autoreset(name):
    assert name in _abi.SIGNATURES
    assert hasattr(_abi.lib(), name)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("on", [0, 1])
def test_null_world_is_invalid_with_a_message(name, on):
    L = _abi.lib()
    assert getattr(L, name)(None, on) == -1  # MACM_E_INVALID
    assert b"NULL" in L.macm_last_error()
