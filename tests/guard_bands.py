"""Output buffers with guard bands, and C-ABI outputs structs built from a subset of fields (tests/ only).

Every buffer handed to the library is the middle of a larger uint8 device allocation: GUARD bytes on
each side, the whole allocation prefilled with FILL. The view starts ALIGN-byte aligned, as a torch
allocation would (the kernels rely on 16 bytes for obs, include/macm.h "Alignment"), so a store before
the first or past the last element lands in a band and is seen, where the allocator's slack around a
plain torch tensor would hide it. The data bytes start as FILL too: a row that a call must not touch
still holds it afterwards."""
import ctypes

import numpy as np
import torch

from gym_macm import _abi
from gym_macm.tdm_world import TdmWorld

GUARD, ALIGN, FILL = 256, 256, 0xA5

FLOCK_FIELDS = ("obs", "nbr_id", "reward", "collided", "done")
TDM_FIELDS = ("obs", "mask", "health", "alive", "done", "winner")


def int_view(t):
    """A float tensor as integers of the same width (its bit patterns); any other tensor as it is."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


class Guarded:
    def __init__(self, shape, dtype, device="cuda:0"):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + 2 * GUARD + ALIGN,), FILL, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.raw.data_ptr() + GUARD)) % ALIGN
        self.bytes = self.raw[self.start:self.start + self.nbytes]
        self.t = self.bytes.view(dtype).view(shape)
        assert self.t.data_ptr() % ALIGN == 0 and self.t.data_ptr() == self.raw.data_ptr() + self.start

    def bands_intact(self) -> bool:
        lo = self.raw[self.start - GUARD:self.start]
        hi = self.raw[self.start + self.nbytes:self.start + self.nbytes + GUARD]
        return bool((lo == FILL).all()) and bool((hi == FILL).all())

    def rows_untouched(self, rows) -> bool:
        """Whether the rows (a bool array over the first axis) still hold the prefill."""
        b = self.bytes.view(self.t.shape[0], -1)
        return bool((b[torch.as_tensor(np.asarray(rows, bool), device=b.device)] == FILL).all())


def field_specs(w) -> dict:
    """field -> (dtype, per-step shape) of a World's or a TdmWorld's outputs."""
    odt = torch.float64 if w.cfg.obs_f64 else torch.float32
    E, N = w.E, w.N
    if isinstance(w, TdmWorld):
        return dict(obs=(odt, (E, N, N - 1, 4)), mask=(torch.uint8, (E, N, N - 1)), health=(torch.float64, (E, N)),
                    alive=(torch.uint8, (E, N)), done=(torch.uint8, (E,)), winner=(torch.int32, (E,)))
    return dict(obs=(odt, (E, N, w.OD)), nbr_id=(torch.int32, (E, N)), reward=(torch.float32, (E, N)),
                collided=(torch.uint8, (E, N)), done=(torch.uint8, (E,)))


class GuardedOutputs:
    """macm_outputs / macm_tdm_outputs of world `w` with the fields in `fields` set to guarded
    buffers and every other field NULL; n_steps: the [n_steps, ...] buffers of the trajectory forms."""

    def __init__(self, w, fields, n_steps=None):
        tdm = isinstance(w, TdmWorld)
        names = TDM_FIELDS if tdm else FLOCK_FIELDS
        assert set(fields) <= set(names), fields
        spec = field_specs(w)
        self.fields = tuple(f for f in names if f in fields)
        self.bufs = {}
        for f in self.fields:
            dt, shp = spec[f]
            self.bufs[f] = Guarded(shp if n_steps is None else (n_steps,) + tuple(shp), dt, w.device)
        ptrs = [ctypes.c_void_p(self.bufs[f].t.data_ptr()) if f in self.bufs else None for f in names]
        self.struct = (_abi.MacmTdmOutputs if tdm else _abi.MacmOutputs)(*ptrs)
        for f in names:  # the fields that are not wanted are NULL in the struct itself
            assert (getattr(self.struct, f) is None) == (f not in self.bufs)

    def ref(self):
        return ctypes.byref(self.struct)

    def __getitem__(self, f):
        return self.bufs[f].t

    def check_bands(self, ctx):
        torch.cuda.synchronize()
        for f, g in self.bufs.items():
            assert g.bands_intact(), f"{ctx}: a store outside the {f} buffer (guard band overwritten)"

    def assert_equal(self, twin: dict, ctx, fields=None):
        """The non-NULL fields (or those of them in `fields`) equal the twin's tensors bit for bit."""
        self.check_bands(ctx)
        for f in self.fields:
            if fields is None or f in fields:
                assert torch.equal(self.bufs[f].t, twin[f]), f"{ctx}: {f} differs from the twin's"
                if f == "obs":  # torch.equal on floats takes -0.0 for +0.0: the bit patterns as well
                    assert torch.equal(int_view(self.bufs[f].t), int_view(twin[f])), f"{ctx}: obs bits differ from the twin's"
