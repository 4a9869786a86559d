"""``ops.mask_moments`` and ``ops.mask_shift``: the Python side of csrc/track.hip (msam_mask_moments, msam_mask_shift).  Defined here and
re-exported by micro_sam_amd/ops.py with the boundary checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``);
tests/test_gpu_track.py runs them on the device.

Bit masks are those of micro_sam_amd/_propagate.py: uint32 [P, ceil(H / 32), W] in int32 storage, bit b of word [p][yw][x] = pixel
(yw * 32 + b, x).  Bits of rows >= H in the last word row of an input are ignored; ``mask_shift`` writes them as zeros."""
from __future__ import annotations

import torch

from . import _lib
from ._propagate import _bits, _shape


def mask_moments(bits: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """int64 [P, 3] = (count, sum of y, sum of x) over the set pixels of every bit mask, exact (msam_mask_moments).  The centre of mass
    is the caller's: ``sums / count`` in fp64 is bit for bit ``np.mean`` of the index arrays of ``np.where(mask == 1)``."""
    from . import ops
    dev = ops._home("bits", bits)
    h, w = _shape(height, width)
    p = _bits("bits", bits, h, w, dev)
    out = torch.empty((p, 3), dtype=torch.int64, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_moments(bits.data_ptr(), p, h, w, out.data_ptr(), _lib.stream_ptr()), "msam_mask_moments")
    return out


def mask_shift(bits: torch.Tensor, height: int, width: int, shifts: torch.Tensor) -> torch.Tensor:
    """Every bit mask moved by its own (sy, sx) of ``shifts`` float64 [P, 2] on the device (msam_mask_shift): a new stack, bit for bit
    ``scipy.ndimage.shift(mask, (sy, sx), order=0, prefilter=False)`` (mode "constant", cval 0) of every mask; a NaN or infinite shift
    gives an empty mask."""
    from . import ops
    dev = ops._home("bits", bits)
    h, w = _shape(height, width)
    p = _bits("bits", bits, h, w, dev)
    ops._t("shifts", shifts, torch.float64, (p, 2), dev)
    out = torch.empty((p, (h + 31) // 32, w), dtype=torch.int32, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_shift(bits.data_ptr(), p, h, w, shifts.data_ptr(), out.data_ptr(), _lib.stream_ptr()),
                   "msam_mask_shift")
    return out
