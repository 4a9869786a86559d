"""``ops.pack_bits``, ``ops.mask_iou_counts``, ``ops.mask_box_prompts``, ``ops.mask_logits`` and ``ops.paint_max``: the Python side of
csrc/propagate.hip (msam_mask_pack, msam_mask_iou_counts, msam_mask_box_prompts, msam_mask_logits, msam_paint_max).  Defined here and
re-exported by micro_sam_amd/ops.py with the boundary checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``);
tests/test_gpu_propagate.py runs them on the device.

Bit masks are uint32 [P, ceil(H / 32), W] in int32 storage, bit b of word [p][yw][x] = pixel (yw * 32 + b, x) - what
``ops.postprocess_masks`` returns as ``bits``.  Bits of rows >= H in the last word row are ignored by every function here."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

MAX_SIDE = 32767                          # include/msam_hip.h MSAM_MASK_MAX_SIDE
MAX_OBJECTS = 65535                       # include/msam_hip.h MSAM_MASK_MAX_OBJECTS


def _shape(height, width) -> Tuple[int, int]:
    from . import ops
    h, w = int(height), int(width)
    ops._need(1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE, f"height and width must lie in [1, {MAX_SIDE}], got {(h, w)}")
    return h, w


def _bits(name: str, bits, h: int, w: int, dev: torch.device, p: Optional[int] = None) -> int:
    from . import ops
    ops._t(name, bits, ops._BITS, (p, (h + 31) // 32, w), dev)
    n = int(bits.shape[0])
    ops._need(n <= MAX_OBJECTS, f"{name} holds {n} masks, at most {MAX_OBJECTS} per call")
    return n


def pack_bits(masks: torch.Tensor) -> torch.Tensor:
    """uint8 / bool [P, H, W] -> bit masks [P, ceil(H / 32), W] (msam_mask_pack): a pixel is set where the value == 1; the tail bits of the
    last word row are zero."""
    from . import ops
    dev = ops._home("masks", masks)
    if isinstance(masks, torch.Tensor) and masks.dtype == torch.bool and masks.is_contiguous():
        masks = masks.view(torch.uint8)
    ops._t("masks", masks, torch.uint8, (None, None, None), dev)
    p = int(masks.shape[0])
    h, w = _shape(masks.shape[1], masks.shape[2])
    ops._need(p <= MAX_OBJECTS, f"masks holds {p} masks, at most {MAX_OBJECTS} per call")
    bits = torch.empty((p, (h + 31) // 32, w), dtype=torch.int32, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_pack(masks.data_ptr(), p, h, w, bits.data_ptr(), _lib.stream_ptr()), "msam_mask_pack")
    return bits


def mask_iou_counts(a: torch.Tensor, b: torch.Tensor, height: int, width: int, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per pair of bit masks a[p], b[p] (msam_mask_iou_counts): counts int32 [P, 2] = (overlap, union), exact, and keep uint8 [P] =
    ``not (util.compute_iou(a[p], b[p]) < threshold)`` in the same fp64 arithmetic."""
    from . import ops
    dev = ops._home("a", a)
    h, w = _shape(height, width)
    p = _bits("a", a, h, w, dev)
    _bits("b", b, h, w, dev, p)
    counts = torch.empty((p, 2), dtype=torch.int32, device=dev)
    keep = torch.empty((p,), dtype=torch.uint8, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_iou_counts(a.data_ptr(), b.data_ptr(), p, h, w, float(threshold), counts.data_ptr(), keep.data_ptr(),
                                                    _lib.stream_ptr()), "msam_mask_iou_counts")
    return counts, keep


def mask_box_prompts(bits: torch.Tensor, height: int, width: int, input_size: Tuple[int, int],
                     box_extension: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Box prompts of bit masks (msam_mask_box_prompts): (nonempty uint8 [P], boxes float32 [P, 4] XYXY in the model's input frame of
    ``input_size`` = (h, w)), bit for bit ``prompt_based_segmentation._compute_box_from_mask(mask, box_extension=...)`` ->
    ``ResizeLongestSide.apply_boxes`` -> float32.  An empty mask has a box of zeros and nonempty = 0."""
    from . import ops
    dev = ops._home("bits", bits)
    h, w = _shape(height, width)
    p = _bits("bits", bits, h, w, dev)
    ih, iw = int(input_size[0]), int(input_size[1])
    ext = float(box_extension)
    ops._need(ih >= 1 and iw >= 1, f"input_size must be positive, got {(ih, iw)}")
    ops._need(0.0 <= ext <= 1e9, f"box_extension must lie in [0, 1e9], got {box_extension}")
    boxes = torch.empty((p, 4), dtype=torch.float32, device=dev)
    nonempty = torch.empty((p,), dtype=torch.uint8, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_box_prompts(bits.data_ptr(), p, h, w, ext, ih, iw, boxes.data_ptr(), nonempty.data_ptr(),
                                                     _lib.stream_ptr()), "msam_mask_box_prompts")
    return nonempty, boxes


def mask_logits(bits: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """Mask prompts of bit masks (msam_mask_logits): float32 [P, 256, 256], what ``prompt_based_segmentation._compute_logits_from_mask``
    gives for every mask - antialiased bilinear resize of the binary mask (longest side -> 256), zero padding, +-log(999) around 0.5.
    Pixels whose resized value lies within rounding of 0.5 may differ from the host's."""
    from . import ops
    dev = ops._home("bits", bits)
    h, w = _shape(height, width)
    p = _bits("bits", bits, h, w, dev)
    logits = torch.empty((p, 256, 256), dtype=torch.float32, device=dev)
    if p:
        _lib.check(_lib.load().msam_mask_logits(bits.data_ptr(), p, h, w, logits.data_ptr(), _lib.stream_ptr()), "msam_mask_logits")
    return logits


def paint_max(bits: torch.Tensor, ids: torch.Tensor, label: torch.Tensor, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``label`` int32 [H, W] (updated in place and returned) = max(label, ids[p]) wherever bit p is set and ``keep[p]`` is non-zero
    (msam_paint_max; ``keep`` None: every object).  ids int32 [P] on the device."""
    from . import ops
    dev = ops._home("bits", bits)
    ops._t("label", label, torch.int32, (None, None), dev)
    h, w = _shape(label.shape[0], label.shape[1])
    p = _bits("bits", bits, h, w, dev)
    ops._t("ids", ids, torch.int32, (p,), dev)
    if keep is not None:
        ops._t("keep", keep, torch.uint8, (p,), dev)
    if p:
        _lib.check(_lib.load().msam_paint_max(bits.data_ptr(), ids.data_ptr(), None if keep is None else keep.data_ptr(), p, h, w,
                                              label.data_ptr(), _lib.stream_ptr()), "msam_paint_max")
    return label
