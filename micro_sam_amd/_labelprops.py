"""``ops.edt_squared``, ``ops.label_props`` and ``ops.distance_targets``: the Python side of csrc/labelprops.hip (msam_edt_squared,
msam_label_props, msam_distance_targets).  Defined here and re-exported by micro_sam_amd/ops.py with the boundary checks of the other
wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); tests/test_gpu_labelprops.py and tests/test_gpu_distance_targets.py run them on the
device."""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional

import torch

from . import _lib

EDT_MAX_SIDE = 32767                      # include/msam_hip.h MSAM_EDT_MAX_SIDE

# per (device, stream): a byte workspace that only grows
_WS: Dict[Any, torch.Tensor] = {}


class LabelProps(NamedTuple):
    """Per object, in the order of ``ids`` (all on the device): ids int32 [N], area int32 [N], bbox int32 [N, 4] (y0, x0, y1, x1,
    exclusive ends), coord_sum int64 [N, 2] (sums of y and x), center int32 [N, 2] (y, x) or None."""
    ids: torch.Tensor
    area: torch.Tensor
    bbox: torch.Tensor
    coord_sum: torch.Tensor
    center: Optional[torch.Tensor]


class DistanceTargets(NamedTuple):
    """``out`` float32 [3, H, W] (foreground, centre distance, boundary distance) and, per object 1..N: ``center`` int32 [N, 2] (y, x),
    ``dmax2`` int32 [N] (the largest squared boundary distance), ``bbox`` int32 [N, 4] (y0, x0, y1, x1, exclusive ends).  All on the device."""
    out: torch.Tensor
    center: torch.Tensor
    dmax2: torch.Tensor
    bbox: torch.Tensor


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _image(name: str, t, dtypes, dev: torch.device):
    from . import ops
    ops._t(name, t, dtypes, (None, None), dev)
    h, w = int(t.shape[0]), int(t.shape[1])
    ops._need(1 <= h <= EDT_MAX_SIDE and 1 <= w <= EDT_MAX_SIDE, f"{name} must be [H, W] with sides in [1, {EDT_MAX_SIDE}], got {list(t.shape)}")
    return h, w


def edt_squared(mask: torch.Tensor) -> torch.Tensor:
    """Exact squared Euclidean distance transform on the device (msam_edt_squared): mask uint8, bool or int32 [H, W], non-zero = inside
    -> int32 [H, W], the squared distance of every pixel to the nearest zero pixel (0 at zero pixels; INT32_MAX everywhere when the mask
    has no zero pixel).  Sides up to 32767."""
    from . import ops
    dev = ops._home("mask", mask)
    if mask.dtype == torch.bool and mask.is_contiguous():
        mask = mask.view(torch.uint8)
    h, w = _image("mask", mask, (torch.uint8, torch.int32), dev)
    lib = _lib.load()
    need = int(lib.msam_edt_squared_workspace_bytes(h, w))
    ws = _workspace(dev, need)
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    _lib.check(lib.msam_edt_squared(mask.data_ptr(), int(mask.dtype == torch.int32), h, w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr()), "msam_edt_squared")
    return out


def label_props(labels: torch.Tensor, ids: Optional[torch.Tensor] = None, centers: bool = True) -> LabelProps:
    """Area, bounding box, coordinate sums and "v" centre of the objects of a label image on the device (msam_label_props): labels int32
    [H, W]; ids int32 [N] positive, distinct and sorted ascending, or None: ``torch.unique`` of the labels on the device without the
    non-positive values.  ``centers=False`` skips the distance transform.  The "v" centre is the object's pixel with the largest exact
    squared distance to the nearest inner boundary of the label image, ties to the first pixel in raster order
    (``util.get_centers_and_bounding_boxes``).  N = 0 returns empty tensors without a launch."""
    from . import ops
    dev = ops._home("labels", labels)
    h, w = _image("labels", labels, torch.int32, dev)
    if ids is None:
        ids = torch.unique(labels)
        ids = ids[ids > 0].contiguous()
    ops._t("ids", ids, torch.int32, (None,), dev)
    n = int(ids.numel())
    ops._need(n < 1 << 31, "ids holds 2^31 entries or more")
    area = torch.empty(n, dtype=torch.int32, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    coord_sum = torch.empty((n, 2), dtype=torch.int64, device=dev)
    center = torch.empty((n, 2), dtype=torch.int32, device=dev) if centers else None
    if n == 0:
        return LabelProps(ids, area, bbox, coord_sum, center)
    lib = _lib.load()
    need = int(lib.msam_label_props_workspace_bytes(h, w, n))
    ws = _workspace(dev, need)
    _lib.check(lib.msam_label_props(labels.data_ptr(), h, w, ids.data_ptr(), n, area.data_ptr(), bbox.data_ptr(), coord_sum.data_ptr(),
                                    None if center is None else center.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "msam_label_props")
    return LabelProps(ids, area, bbox, coord_sum, center)


def distance_targets(labels: torch.Tensor, n_objects: Optional[int] = None, correct_centers: bool = True, fill: float = 1.0) -> DistanceTargets:
    """The training targets of the convolutional decoder on the device (msam_distance_targets; torch_em's ``PerObjectDistanceTransform``
    restated, UNPINNED - torch_em is not available; definitions in include/msam_hip.h and DESIGN.md 8.4): labels int32 [H, W] whose
    objects are the consecutive labels 1..``n_objects`` (every other value is background; None: the maximum of the labels, which costs one
    synchronisation) -> ``DistanceTargets``.  Background pixels hold ``fill`` in the two distance planes.  Integer work is exact and
    two calls agree bit for bit."""
    from . import ops
    dev = ops._home("labels", labels)
    h, w = _image("labels", labels, torch.int32, dev)
    n = max(int(labels.max()), 0) if n_objects is None else int(n_objects)
    ops._need(0 <= n < 1 << 31, f"n_objects must be in [0, 2^31), got {n}")
    ops._need(fill == fill, "fill is NaN")
    out = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    center = torch.empty((n, 2), dtype=torch.int32, device=dev)
    dmax2 = torch.empty(n, dtype=torch.int32, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = int(lib.msam_distance_targets_workspace_bytes(h, w, n))
    ws = _workspace(dev, need)
    _lib.check(lib.msam_distance_targets(labels.data_ptr(), h, w, n, int(bool(correct_centers)), float(fill), out.data_ptr(),
                                         center.data_ptr() if n else None, dmax2.data_ptr() if n else None, bbox.data_ptr() if n else None,
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "msam_distance_targets")
    return DistanceTargets(out, center, dmax2, bbox)
