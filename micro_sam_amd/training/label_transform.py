"""``PerObjectDistanceTransform``: the label transform behind the targets of the convolutional (UNETR) decoder - foreground, normalised
distance to the object centre, normalised distance to the object boundary - with its per-object work on the device
(``ops.distance_targets``, csrc/labelprops.hip).

PARITY UNPINNED.  The reference trains the decoder on ``torch_em.transform.label.PerObjectDistanceTransform``; torch_em is neither
vendored in the reference nor installed here, so the transform is restated from its published source, with the same standing as
``models/unetr.py``.  The definitions this file and the kernel implement are written out in include/msam_hip.h and DESIGN.md 8.4;
tests/distance_targets_ref.py restates torch_em's per-object loop (crop, distance transform, vector distance transform per object) and
the tests compare the two.

Where it runs: the per-object loop is the known bottleneck of the reference's data-loader workers on patches with hundreds of cells.
Here one call handles all objects of a patch on the device - which means the transform belongs IN THE TRAINING PROCESS (``JointSamTrainer``
applies it to a loader's raw instance labels), not in forked data-loader workers: a forked worker must not touch the GPU.
"""
from __future__ import annotations

from typing import Union

import numpy as np
import torch

from .._labelprops import DistanceTargets  # noqa: F401  (the type ``_distance_targets`` returns)


def label_components(labels: np.ndarray) -> np.ndarray:
    """``skimage.measure.label`` with its defaults (scikit-image is not available: restated, unpinned): connected components of equal
    non-zero value under 8-connectivity, numbered from 1 by their first pixel in raster order; 0 stays background.  On the host, as in the
    reference: the union-find of ``scipy.sparse.csgraph.connected_components`` over the equal-valued neighbour pairs is exact."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    lab = np.asarray(labels)
    if lab.ndim != 2:
        raise NotImplementedError(f"label_components: 2-d label images only, got {lab.ndim}-d (3-d labels are not implemented)")
    h, w = lab.shape
    idx = np.arange(h * w).reshape(h, w)
    rows, cols = [], []
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:-1, :-1], np.s_[1:, 1:]), (np.s_[:-1, 1:], np.s_[1:, :-1])):
        same = (lab[a] == lab[b]) & (lab[a] != 0)
        rows.append(idx[a][same]); cols.append(idx[b][same])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(h * w, h * w))
    _, comp = connected_components(graph, directed=False)
    fg = lab.reshape(-1) != 0
    out = np.zeros(h * w, np.int32)
    if fg.any():
        # components in the order of their first pixel: np.unique returns the first index of every value
        _, first, inverse = np.unique(comp[fg], return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(1, len(first) + 1)
        out[fg] = rank[inverse.reshape(-1)]
    return out.reshape(h, w)


def _device(labels) -> torch.device:
    from .. import _lib
    return labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else _lib.require_gpu()


def _distance_targets(labels: torch.Tensor, n_objects: int, correct_centers: bool, fill: float) -> "DistanceTargets":
    from .. import ops
    return ops.distance_targets(labels, n_objects=n_objects, correct_centers=correct_centers, fill=fill)


class PerObjectDistanceTransform:
    """torch_em's ``PerObjectDistanceTransform`` (signature and channel order as there; unpinned, see the module docstring).

    ``__call__(labels)``: a 2-d label image, numpy array or tensor -> float32 ``[C, H, W]`` of the same kind (a numpy array for an array;
    for a tensor, a tensor on the device the work ran on).  Channels, each only if its flag is set: ``[instances, foreground, centre
    distances, boundary distances]``.

    Steps: ``apply_label`` relabels by connected components on the HOST (``label_components``; a device tensor is downloaded for this
    step and the result uploaded); objects smaller than ``min_size`` become background and the remaining ids are made consecutive in
    ascending order, both as torch operators on the device; ``ops.distance_targets`` computes the channels for all objects at once.
    Background pixels of the distance channels hold ``distance_fill_value``.

    Not implemented: ``directed_distances`` (the two signed components of the vector to the centre) and 3-d label volumes.

    The transform uses the GPU: call it in the training process, never in forked data-loader workers."""

    eps = 1e-7

    def __init__(self, distances: bool = True, boundary_distances: bool = True, directed_distances: bool = False, foreground: bool = True,
                 instances: bool = False, apply_label: bool = True, correct_centers: bool = True, min_size: int = 0,
                 distance_fill_value: float = 1.0) -> None:
        if directed_distances:
            raise NotImplementedError("PerObjectDistanceTransform: directed_distances (the signed components of the vector to the object "
                                      "centre) are not implemented; only the undirected centre distance is")
        self.distances, self.boundary_distances, self.directed_distances = bool(distances), bool(boundary_distances), False
        self.foreground, self.instances = bool(foreground), bool(instances)
        self.apply_label, self.correct_centers = bool(apply_label), bool(correct_centers)
        self.min_size, self.distance_fill_value = int(min_size), float(distance_fill_value)

    def __call__(self, labels: Union[np.ndarray, torch.Tensor]) -> Union[np.ndarray, torch.Tensor]:
        is_tensor = isinstance(labels, torch.Tensor)
        if labels.ndim != 2:
            raise NotImplementedError(f"PerObjectDistanceTransform: 2-d label images only, got {labels.ndim}-d (3-d label volumes are not implemented)")
        dev = _device(labels)
        if self.apply_label:
            host = labels.detach().cpu().numpy() if is_tensor else np.asarray(labels)
            lab = torch.from_numpy(label_components(host)).to(dev)
        else:
            lab = (labels if is_tensor else torch.from_numpy(np.ascontiguousarray(labels))).to(dev)
            lab = lab.round().to(torch.int64) if lab.is_floating_point() else lab.to(torch.int64)
        lab, n = self._filter_and_relabel(lab)
        t = _distance_targets(lab, n, self.correct_centers, self.distance_fill_value)
        channels = []
        if self.instances:
            channels.append(lab.to(torch.float32)[None])
        if self.foreground:
            channels.append(t.out[0:1])
        if self.distances:
            channels.append(t.out[1:2])
        if self.boundary_distances:
            channels.append(t.out[2:3])
        out = torch.cat(channels, dim=0) if channels else torch.empty((0, *lab.shape), dtype=torch.float32, device=dev)
        return out if is_tensor else out.cpu().numpy()

    def _filter_and_relabel(self, lab: torch.Tensor):
        """Objects below ``min_size`` -> background; the remaining positive ids -> 1..N in ascending order.  -> (int32 [H, W], N)."""
        ids, inverse, sizes = torch.unique(lab, return_inverse=True, return_counts=True)      # ascending
        keep = ids > 0
        if self.min_size > 0:
            keep &= sizes >= self.min_size
        new_id = torch.cumsum(keep, 0) * keep                            # kept id -> its rank among the kept ids, everything else -> 0
        return new_id[inverse].to(torch.int32).contiguous(), int(keep.sum())
