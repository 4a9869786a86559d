"""``ops.seed_centers``: the Python side of msam_seed_centers (csrc/labelprops.hip), the prompt derivation of the reference's
``AutomaticPromptGenerator`` on the device.  Defined here and re-exported by micro_sam_amd/ops.py with the boundary checks of the other
wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); tests/test_gpu_prompt_seeds.py runs it on the device,
tests/test_prompt_seeds_boundary_host.py checks the boundary."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._labelprops import EDT_MAX_SIDE, _workspace          # (the per-(device, stream) workspace of the other entries of labelprops.hip)


class SeedCenters(NamedTuple):
    """``n`` components; ``undefined``: some component pixel sees no zero pixel inside its block's window, where the reference's distance
    transform is not defined (the centres are then unspecified); ``centers`` int32 [n, 2] (y, x) on the device, in component order."""
    n: int
    undefined: bool
    centers: torch.Tensor


def _threshold(name: str, value) -> float:
    """The fp64 number the kernel compares the float32 map with, so that the outcome is numpy's ``map < value`` for the installed numpy:
    numpy compares in ``result_type(map, value)``, which rounds a Python float to float32 first and leaves a ``np.float64`` scalar as it
    is (NEP 50); a float32 widened to fp64 compares as the float32 does."""
    from . import ops
    ops._need(isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, (bool, np.bool_)),
              f"{name} must be a real number, got {type(value).__name__}")
    dt = np.result_type(np.empty(1, np.float32), value)
    ops._need(dt in (np.dtype(np.float32), np.dtype(np.float64)), f"{name}: numpy compares a float32 map with it in {dt}, the kernel cannot")
    with np.errstate(over="ignore"):
        v = float(np.asarray(value).astype(dt))
    ops._need(v == v, f"{name} is NaN")
    return v


def seed_centers(foreground: torch.Tensor, center_distances: torch.Tensor, boundary_distances: torch.Tensor,
                 foreground_threshold=0.5, center_distance_threshold=0.5, boundary_distance_threshold=0.5,
                 avoid_image_border: bool = True) -> SeedCenters:
    """One centre per seed component of the decoder maps on the device (msam_seed_centers; reference ``_derive_point_prompts`` +
    ``_get_centers``, contract in include/msam_hip.h and DESIGN.md 8.11): the three maps float32 [H, W] with sides up to 32767 ->
    ``SeedCenters``.  The thresholds compare as numpy compares a float32 array with them.  Only the four words of the result record
    are read back (one synchronisation); no pixel data leaves the device."""
    from . import ops
    dev = ops._home("foreground", foreground)
    ops._t("foreground", foreground, torch.float32, (None, None), dev)
    h, w = int(foreground.shape[0]), int(foreground.shape[1])
    ops._need(1 <= h <= EDT_MAX_SIDE and 1 <= w <= EDT_MAX_SIDE,
              f"foreground must be [H, W] with sides in [1, {EDT_MAX_SIDE}], got {list(foreground.shape)}")
    ops._t("center_distances", center_distances, torch.float32, (h, w), dev)
    ops._t("boundary_distances", boundary_distances, torch.float32, (h, w), dev)
    ft = _threshold("foreground_threshold", foreground_threshold)
    ct = _threshold("center_distance_threshold", center_distance_threshold)
    bt = _threshold("boundary_distance_threshold", boundary_distance_threshold)
    cap = (h * w + 1) // 2                                   # no two seed pixels that share an edge lie in different components
    lib = _lib.load()
    ws = _workspace(dev, int(lib.msam_seed_centers_workspace_bytes(h, w, cap)))
    centers = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    result = torch.zeros(4, dtype=torch.int32, device=dev)
    _lib.check(lib.msam_seed_centers(foreground.data_ptr(), center_distances.data_ptr(), boundary_distances.data_ptr(), h, w, ft, ct, bt,
                                     int(bool(avoid_image_border)), centers.data_ptr(), cap, result.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr()), "msam_seed_centers")
    n, undefined, incomplete, _ = (int(v) for v in result.tolist())
    if incomplete:
        raise RuntimeError("micro_sam_amd: msam_seed_centers: the component labelling did not complete")
    return SeedCenters(n, bool(undefined), centers[:n].clone())           # (the buffer for the largest possible N is let go)
