"""tests/guard_bands.py itself, on host memory (no GPU): the view is 256-byte aligned inside its
allocation, a byte stored just before or just past it is reported, and rows that were not written
still count as untouched. A helper that reported nothing would make every guard-band test pass."""
import numpy as np
import pytest
import torch

from guard_bands import ALIGN, FILL, GUARD, Guarded


@pytest.mark.parametrize("shape,dtype", [((3, 5, 4), torch.float32), ((3, 5, 4), torch.float64), ((7,), torch.uint8),
                                         ((2, 3, 9), torch.int32), ((1, 1025, 1024), torch.uint8)])
def test_bands_report_a_store_outside_the_view(shape, dtype):
    g = Guarded(shape, dtype, device="cpu")
    assert g.t.data_ptr() % ALIGN == 0 and tuple(g.t.shape) == shape and g.t.dtype == dtype
    assert g.start >= GUARD and g.start + g.nbytes + GUARD <= g.raw.numel()
    assert g.bands_intact() and g.rows_untouched(np.ones(shape[0], bool))
    g.t.zero_()  # everything inside the view: the bands stay
    assert g.bands_intact() and not g.rows_untouched(np.ones(shape[0], bool))
    for off in (g.start - 1, g.start - GUARD, g.start + g.nbytes, g.start + g.nbytes + GUARD - 1):
        g.raw[off] = 0
        assert not g.bands_intact(), off
        g.raw[off] = FILL
        assert g.bands_intact()


def test_rows_untouched_sees_single_rows():
    g = Guarded((4, 6), torch.int32, device="cpu")
    g.t[2, 5] = 7
    assert g.rows_untouched([True, True, False, True]) and not g.rows_untouched([False, False, True, False])
