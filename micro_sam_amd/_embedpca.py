"""``ops.pca_moments``, ``ops.pca_project`` and ``ops.pca_to_rgb``: the Python side of csrc/embedpca.hip (msam_pca_moments,
msam_pca_project, msam_pca_to_rgb).  Defined here and re-exported by micro_sam_amd/ops.py with the boundary checks of the other wrappers
(``ops._home`` / ``ops._t`` / ``ops._need``); every check runs before the first launch.  tests/test_visualization_host.py and
tests/test_gpu_visualization.py run them."""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch

from . import _lib

PCA_MAX_UNITS, PCA_MAX_CHANNELS, PCA_MAX_COMPONENTS = 65535, 256, 8        # include/msam_hip.h MSAM_PCA_*

# per (device, stream): a byte workspace that only grows
_WS: Dict[Any, torch.Tensor] = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _units(name: str, x, dev: torch.device) -> Tuple[int, int, int]:
    from . import ops
    ops._t(name, x, torch.float32, (None, None, None), dev)
    u, c, n = (int(v) for v in x.shape)
    ops._need(1 <= u <= PCA_MAX_UNITS and 1 <= c <= PCA_MAX_CHANNELS and n >= 1 and c * n < 2 ** 31,
              f"{name} must be [1..{PCA_MAX_UNITS}, 1..{PCA_MAX_CHANNELS}, N >= 1] with C * N < 2^31, got {list(x.shape)}")
    return u, c, n


def pca_moments_workspace_bytes(units: int, channels: int, positions: int) -> int:
    """Bytes of workspace ``pca_moments`` needs for ``units`` embeddings of [channels, positions] (msam_pca_moments_workspace_bytes)."""
    return int(_lib.load().msam_pca_moments_workspace_bytes(int(units), int(channels), int(positions)))


def pca_moments(x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Channel means and centred Gram matrices of U embeddings on the device (msam_pca_moments): x float32 [U, C, N], contiguous, C <= 256
    -> mean float32 [U, C] and gram float64 [U, C, C] = sum_n (x_n - mean)(x_n - mean)^T, exactly symmetric.  ``workspace``: a flat uint8
    tensor of at least ``pca_moments_workspace_bytes(U, C, N)`` bytes (None: one kept per device and stream).  Two calls agree bit for bit,
    and a unit's result does not depend on the other units of the call."""
    from . import ops
    dev = ops._home("x", x)
    u, c, n = _units("x", x, dev)
    lib = _lib.load()
    need = int(lib.msam_pca_moments_workspace_bytes(u, c, n))
    if workspace is None:
        workspace = _workspace(dev, need)
    else:
        ops._blob("workspace", workspace, need, dev)
        ops._need(workspace.data_ptr() % 8 == 0, "workspace must be 8-byte aligned")
    mean = torch.empty((u, c), dtype=torch.float32, device=dev)
    gram = torch.empty((u, c, c), dtype=torch.float64, device=dev)
    _lib.check(lib.msam_pca_moments(x.data_ptr(), u, c, n, mean.data_ptr(), gram.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                    _lib.stream_ptr()), "msam_pca_moments")
    return mean, gram


def pca_project(x: torch.Tensor, components: torch.Tensor, mean: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Projection of U embeddings onto K <= 8 components each (msam_pca_project): x float32 [U, C, N], components float32 [U, K, C], mean
    float32 [U, C] -> out float32 [U, K, N] = components @ (x - mean), summed over the channels in ascending order, and minmax float32
    [U, 2], the minimum and maximum of every unit's K * N values."""
    from . import ops
    dev = ops._home("x", x)
    u, c, n = _units("x", x, dev)
    ops._t("components", components, torch.float32, (u, None, c), dev)
    k = int(components.shape[1])
    ops._need(1 <= k <= PCA_MAX_COMPONENTS, f"components must hold 1 to {PCA_MAX_COMPONENTS} rows per unit, got {list(components.shape)}")
    ops._t("mean", mean, torch.float32, (u, c), dev)
    out = torch.empty((u, k, n), dtype=torch.float32, device=dev)
    minmax = torch.empty((u, 2), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().msam_pca_project(x.data_ptr(), components.data_ptr(), mean.data_ptr(), u, c, n, k, out.data_ptr(),
                                            minmax.data_ptr(), _lib.stream_ptr()), "msam_pca_project")
    return out, minmax


def pca_to_rgb(proj: torch.Tensor, minmax: torch.Tensor) -> torch.Tensor:
    """uint8 [U, N, 3] = trunc((255 * (proj - min)) / (max - min)) in fp32 (msam_pca_to_rgb) from proj float32 [U, 3, N] and minmax float32
    [U, 2]; a unit with max == min gives zeros."""
    from . import ops
    dev = ops._home("proj", proj)
    ops._t("proj", proj, torch.float32, (None, 3, None), dev)
    u, _, n = (int(v) for v in proj.shape)
    ops._need(1 <= u <= PCA_MAX_UNITS and n >= 1 and 3 * n < 2 ** 31, f"proj must be [1..{PCA_MAX_UNITS}, 3, N] with 1 <= 3 N < 2^31, got {list(proj.shape)}")
    ops._t("minmax", minmax, torch.float32, (u, 2), dev)
    rgb = torch.empty((u, n, 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().msam_pca_to_rgb(proj.data_ptr(), minmax.data_ptr(), u, n, rgb.data_ptr(), _lib.stream_ptr()), "msam_pca_to_rgb")
    return rgb
