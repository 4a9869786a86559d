"""``ops.close_gaps_z``, ``ops.label_z_ranges`` and ``ops.apply_label_lut``: the Python side of csrc/merge3d.hip (msam_close_gaps,
msam_label_z_ranges, msam_apply_label_lut), the passes over a label volume around the multicut of
``multi_dimensional_segmentation.merge_instance_segmentation_3d``.  Defined here and re-exported by micro_sam_amd/ops.py with the
boundary checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); tests/test_gpu_merge3d.py runs them on the device,
tests/test_merge3d_boundary_host.py checks the boundary.

Label volumes are int32 [Z, H, W], contiguous.  Nothing here reads a result back: flags come back as device tensors, the caller decides
when to look at them."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib


def _volume(name: str, labels, dev) -> Tuple[int, int, int]:
    from . import ops
    ops._t(name, labels, torch.int32, (None, None, None), dev)
    z, h, w = (int(s) for s in labels.shape)
    ops._need(h * w < 2 ** 31 and z * h * w < 2 ** 38, f"{name} must hold fewer than 2^31 pixels per slice and 2^38 in all, got {list(labels.shape)}")
    return z, h, w


def _count(name: str, value, lo: int, hi: int) -> int:
    from . import ops
    ops._need(isinstance(value, int) and not isinstance(value, bool), f"{name} must be an int, got {type(value).__name__}")
    ops._need(lo <= value <= hi, f"{name} must lie in [{lo}, {hi}], got {value}")
    return value


def close_gaps_z(labels: torch.Tensor, gap: int, id_limit: Optional[int] = None, workspace: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``multi_dimensional_segmentation._preprocess_closing(labels, gap)`` on the device, integer for integer (msam_close_gaps; contract
    in include/msam_hip.h): labels int32 [Z, H, W] with values >= 0 -> (out int32 [Z, H, W], result int32 [4] on the
    device = final running offset, label-outside-the-range flag, labelling-incomplete flag, 0).  ``id_limit`` must be larger than
    every label (None: the volume's maximum + 1, which reads one number back); ``workspace``: a uint8 tensor of at least
    ``msam_close_gaps_workspace_bytes`` (None: allocated here).  An empty volume comes back as it is, without a launch."""
    from . import ops
    dev = ops._home("labels", labels)
    z, h, w = _volume("labels", labels, dev)
    gap = _count("gap", gap, 1, 2 ** 31 - 1)
    if id_limit is not None:
        id_limit = _count("id_limit", id_limit, 1, 2 ** 31 - 1)
    if workspace is not None:
        ops._t("workspace", workspace, torch.uint8, (None,), dev)
    result = torch.zeros(4, dtype=torch.int32, device=dev)
    if labels.numel() == 0:
        result[0] = 1
        return torch.empty_like(labels), result
    if id_limit is None:
        id_limit = max(int(labels.max()), 0) + 1
    lib = _lib.load()
    need = int(lib.msam_close_gaps_workspace_bytes(z, h, w, gap, id_limit))
    ops._need(need > 0, f"labels {list(labels.shape)} with gap {gap} and id_limit {id_limit} is more than msam_close_gaps takes")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ops._need(workspace.numel() >= need, f"workspace holds {workspace.numel()} bytes, msam_close_gaps needs {need}")
    ops._need(workspace.data_ptr() % 4 == 0, "workspace must start on a 4-byte boundary")
    out = torch.empty_like(labels)
    _lib.check(lib.msam_close_gaps(labels.data_ptr(), z, h, w, gap, id_limit, out.data_ptr(), result.data_ptr(), workspace.data_ptr(),
                                   workspace.numel(), _lib.stream_ptr()), "msam_close_gaps")
    return out, result


def label_z_ranges(labels: torch.Tensor, n_ids: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(zr int32 [n_ids, 2], flag int32 [1]) on the device (msam_label_z_ranges): the smallest and the largest slice every id occurs
    in, (Z, -1) for an id that never occurs and for the background id 0; ``flag`` is 1 when a label lies outside [0, n_ids)."""
    from . import ops
    dev = ops._home("labels", labels)
    z, h, w = _volume("labels", labels, dev)
    n_ids = _count("n_ids", n_ids, 1, 2 ** 30)
    zr = torch.empty((n_ids, 2), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if labels.numel() == 0:
        zr[:, 0], zr[:, 1] = z, -1
        return zr, flag
    _lib.check(_lib.load().msam_label_z_ranges(labels.data_ptr(), z, h, w, n_ids, zr.data_ptr(), flag.data_ptr(), _lib.stream_ptr()),
               "msam_label_z_ranges")
    return zr, flag


def apply_label_lut(labels: torch.Tensor, lut: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(``lut[labels]``, flag int32 [1]) on the device (msam_apply_label_lut): labels int32 of any shape, lut int32 [n]; where a label
    lies outside [0, n), 0 is written and ``flag`` is 1.  ``out``: where to write (may be ``labels`` itself); None: a new tensor."""
    from . import ops
    dev = ops._home("labels", labels)
    ops._t("labels", labels, torch.int32, None, dev)
    ops._need(labels.numel() < 2 ** 38, f"labels must hold fewer than 2^38 values, got {list(labels.shape)}")
    ops._t("lut", lut, torch.int32, (None,), dev)
    ops._need(1 <= lut.numel() < 2 ** 31, f"lut must hold between 1 and 2^31 - 1 entries, got {lut.numel()}")
    if out is None:
        out = torch.empty_like(labels)
    else:
        ops._t("out", out, torch.int32, tuple(labels.shape), dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if labels.numel():
        _lib.check(_lib.load().msam_apply_label_lut(labels.data_ptr(), labels.numel(), lut.data_ptr(), lut.numel(), out.data_ptr(),
                                                    flag.data_ptr(), _lib.stream_ptr()), "msam_apply_label_lut")
    return out, flag
