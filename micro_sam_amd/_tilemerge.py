"""``ops.tiled_mask_overlaps`` and ``ops.paint_tiled``: the Python side of csrc/tilemerge.hip (msam_tiled_mask_overlaps, msam_paint_tiled).
Defined here and re-exported by micro_sam_amd/ops.py with the boundary checks of the other wrappers (``ops._home`` / ``ops._t`` /
``ops._need``); tests/test_gpu_tiled_merge.py runs them on the device.

Both read a record table: ``words``, the flat device buffer of the bit masks of all tiles (each [n, ceil(th / 32), tw] as ``ops.pack_bits``
writes them), and per record its first word (``word_offset`` int64 [K]) and ``geom`` int32 [K, 8] = wpc, tw, bx, by, bw, bh, gx, gy (words
per column and width of the record's tile, its ``bbox`` xywh in the tile, the first two entries of its ``global_bbox``).  ``word_offset``,
``geom`` and the index lists are HOST arrays: what the kernels take on trust about them is checked here, before the upload."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def _table(words, word_offset, geom, dev: torch.device):
    """Checks of the table both kernels rely on; returns (K, word_offset, geom) on the device."""
    from . import ops
    ops._t("words", words, ops._BITS, (None,), dev)
    ops._need(isinstance(geom, np.ndarray) and geom.dtype == np.int32 and geom.ndim == 2 and geom.shape[1] == 8,
              "geom must be a host int32 array [K, 8]")
    k = int(geom.shape[0])
    ops._need(isinstance(word_offset, np.ndarray) and word_offset.dtype == np.int64 and word_offset.shape == (k,),
              f"word_offset must be a host int64 array [{k}] like geom")
    g = geom.astype(np.int64)
    wpc, tw, bx, by, bw, bh = (g[:, c] for c in range(6))
    ops._need(bool(np.all((wpc >= 1) & (tw >= 1) & (bw >= 0) & (bh >= 0))), "geom holds an empty tile or a negative bbox size")
    ops._need(bool(np.all((bx >= 0) & (bx + bw <= tw) & (by >= 0) & (by + bh <= 32 * wpc))), "geom holds a bbox that leaves its tile")
    ops._need(bool(np.all((word_offset >= 0) & (word_offset + wpc * tw <= int(words.numel())))),
              "word_offset points outside words")
    return k, torch.from_numpy(np.ascontiguousarray(word_offset)).to(dev), torch.from_numpy(np.ascontiguousarray(geom)).to(dev)


def tiled_mask_overlaps(words: torch.Tensor, word_offset: np.ndarray, geom: np.ndarray, pairs: np.ndarray) -> torch.Tensor:
    """Per pair (i, j) of ``pairs`` (host int32 [Np, 2]) the number of pixels set in both records' masks inside the intersection window
    of their global xywh boxes (msam_tiled_mask_overlaps; reference ``util._calculate_tiled_mask_overlap_matrix``): int32 [Np] on the
    device.  One launch over the listed pairs."""
    from . import ops
    dev = ops._home("words", words)
    k, off_d, geom_d = _table(words, word_offset, geom, dev)
    ops._need(isinstance(pairs, np.ndarray) and pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2,
              "pairs must be a host int32 array [Np, 2]")
    ops._need(bool(np.all((pairs >= 0) & (pairs < k))), f"pairs names records outside [0, {k})")
    n = int(pairs.shape[0])
    inter = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        pairs_d = torch.from_numpy(np.ascontiguousarray(pairs)).to(dev)
        _lib.check(_lib.load().msam_tiled_mask_overlaps(words.data_ptr(), off_d.data_ptr(), geom_d.data_ptr(), k, pairs_d.data_ptr(), n,
                                                        inter.data_ptr(), _lib.stream_ptr()), "msam_tiled_mask_overlaps")
    return inter


def paint_tiled(words: torch.Tensor, word_offset: np.ndarray, geom: np.ndarray, order: np.ndarray, height: int, width: int) -> torch.Tensor:
    """The paint step of ``util.mask_data_to_segmentation(..., merge_exclusively=True)`` for tile-local records (msam_paint_tiled): record
    ``order[r]`` (host int32 [M]) paints M - r through its global box wherever its mask is set and the FIRST record of ``order`` that
    covers a pixel wins; int32 [height, width] on the device, 0 where nothing painted."""
    from . import ops
    dev = ops._home("words", words)
    k, off_d, geom_d = _table(words, word_offset, geom, dev)
    h, w = int(height), int(width)
    ops._need(h >= 1 and w >= 1 and h * w < 2 ** 31, f"height and width must be positive with fewer than 2^31 pixels, got {(h, w)}")
    ops._need(isinstance(order, np.ndarray) and order.dtype == np.int32 and order.ndim == 1, "order must be a host int32 array [M]")
    ops._need(bool(np.all((order >= 0) & (order < k))), f"order names records outside [0, {k})")
    g = geom.astype(np.int64)
    ops._need(bool(np.all((g[:, 6] >= 0) & (g[:, 6] + g[:, 4] <= w) & (g[:, 7] >= 0) & (g[:, 7] + g[:, 5] <= h))),
              f"geom holds a global box that leaves the image {(h, w)}")
    m = int(order.shape[0])
    label = torch.empty((h, w), dtype=torch.int32, device=dev)
    order_d = torch.from_numpy(np.ascontiguousarray(order)).to(dev) if m else None
    _lib.check(_lib.load().msam_paint_tiled(words.data_ptr() if m else None, off_d.data_ptr() if m else None,
                                            geom_d.data_ptr() if m else None, order_d.data_ptr() if m else None, m, h, w,
                                            label.data_ptr(), _lib.stream_ptr()), "msam_paint_tiled")
    return label
