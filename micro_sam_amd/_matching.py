"""``ops.label_matching``: the Python side of msam_label_matching (csrc/matching.hip).  It is defined here and re-exported by
micro_sam_amd/ops.py with the boundary checks of the other wrappers (``ops._home`` / ``ops._need`` / a dtype check that raises
TypeError); tests/test_evaluation_host.py and tests/test_gpu_evaluation.py run its single-fault refusals."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MATCH_HEADER, MATCH_ITEM, MATCH_EDGE, MATCH_MAX_THRESHOLDS, MATCH_MAX_BATCH = 4, 20, 6, 16, 65535      # include/msam_hip.h MSAM_MATCH_*
_MIN_CAPACITY, _MAX_CAPACITY = 1 << 13, 1 << 24

# per (device, stream): [workspace, capacity, result, max_edges]; sizes that had to grow stay grown
_MATCH_WS: Dict[Any, list] = {}


def label_matching(pred: torch.Tensor, gt: torch.Tensor, thresholds: Sequence[float]) -> List[Tuple[int, int, np.ndarray, np.ndarray]]:
    """Score ``B`` predicted label images against ground truth on the device (msam_label_matching): pred int32 [B,H,W]; gt int32
    [B,H,W], or [1,H,W] to score every prediction against one image (the grid search).  Ids: non-negative, 0 = background.
    ``thresholds``: 1 to 16 floats.  One library call (three kernels) and ONE device-to-host copy of one packed buffer; the hash tables
    and the edge list are enlarged and the call repeated when they overflow, as ``slice_overlaps`` does.

    Returns per batch item ``(n_pred, n_true, counts, edges)``: the numbers of distinct non-zero ids, int64 [T] numbers of (pred, gt)
    pairs with IoU >= t, and the int64 [E, 5] rows (pred id, gt id, common pixels, pred area, gt area) of the pairs with IoU >= min(t),
    sorted by (pred id, gt id).  IoU = c / max(area_p + area_g - c, 1e-7) in fp64, the division elf.evaluation.matching performs."""
    from . import ops
    dev = ops._home("pred", pred)
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"micro_sam_amd: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise TypeError(f"micro_sam_amd: {name} must be int32, got {t.dtype}")
        ops._need(t.dim() == 3, f"{name} must be [B,H,W], got {list(t.shape)}")
        ops._need(t.is_contiguous(), f"{name} must be contiguous, got shape {list(t.shape)} with strides {t.stride()}")
        ops._need(t.device == dev, f"{name} lives on {t.device}, pred on {dev}")
    b, h, w = (int(v) for v in pred.shape)
    g = int(gt.shape[0])
    ops._need(1 <= b <= MATCH_MAX_BATCH and h > 0 and w > 0 and h * w < 2 ** 31, f"pred must be [1..65535, H, W] with 0 < H * W < 2^31, got {list(pred.shape)}")
    ops._need(g in (1, b) and tuple(gt.shape[1:]) == (h, w), f"gt must be [{b}, {h}, {w}] or [1, {h}, {w}], got {list(gt.shape)}")
    thr = [float(t) for t in np.asarray(thresholds, dtype=np.float64).reshape(-1)]
    ops._need(1 <= len(thr) <= MATCH_MAX_THRESHOLDS and not any(np.isnan(thr)), f"thresholds must be 1 to 16 numbers, got {len(thr)}")
    c_thr = (C.c_double * len(thr))(*thr)
    lib = _lib.load()
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    state = _MATCH_WS.get(key)
    if state is None:
        state = _MATCH_WS[key] = [None, _MIN_CAPACITY, None, 0]
    while True:
        cap = state[1]
        while b * cap > 2 ** 31:
            raise RuntimeError(f"label_matching: {b} images with tables of {cap} slots exceed 2^31 slots; score fewer images per call")
        max_edges = max(state[3], 4096, 512 * b)
        need = int(lib.msam_label_matching_workspace_bytes(b, cap))
        n_res = MATCH_HEADER + b * MATCH_ITEM + max_edges * MATCH_EDGE
        if state[0] is None or state[0].numel() < need or state[0].device != dev:
            state[0] = torch.empty(need, dtype=torch.uint8, device=dev)
        if state[2] is None or state[2].numel() < n_res or state[2].device != dev:
            state[2] = torch.empty(n_res, dtype=torch.int32, device=dev)
        ws, res = state[0], state[2]
        _lib.check(lib.msam_label_matching(pred.data_ptr(), gt.data_ptr(), b, g, h, w, c_thr, len(thr), ws.data_ptr(), ws.numel(), cap,
                                           res.data_ptr(), max_edges, _lib.stream_ptr()), "msam_label_matching")
        out = res[:n_res].cpu().numpy()
        items = out[MATCH_HEADER:MATCH_HEADER + b * MATCH_ITEM].reshape(b, MATCH_ITEM)
        n_edges = int(out[0])
        table_full, list_full = bool(items[:, 3].any()), bool(out[1]) or n_edges > max_edges
        if not table_full and not list_full:
            break
        if table_full:
            if cap >= _MAX_CAPACITY:
                raise RuntimeError(f"label_matching: more than {_MAX_CAPACITY} slots per image would be needed")
            state[1] = cap * 4
        if list_full:
            state[3] = max(2 * max_edges, n_edges)
    edges = out[MATCH_HEADER + b * MATCH_ITEM:].reshape(max_edges, MATCH_EDGE)[:n_edges].astype(np.int64)
    edges = edges[np.lexsort((edges[:, 2], edges[:, 1], edges[:, 0]))]
    starts = np.searchsorted(edges[:, 0], np.arange(b + 1))
    return [(int(items[i, 0]), int(items[i, 1]), items[i, 4:4 + len(thr)].astype(np.int64), edges[starts[i]:starts[i + 1], 1:])
            for i in range(b)]
