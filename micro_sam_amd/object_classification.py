"""Object features from SAM embeddings and object classification (reference micro_sam/object_classification.py).

``compute_object_features`` restates ``_compute_object_features_impl`` (object_classification.py:20-57) - pad the label image to a
square, resize the 64 x 64 x 256 embedding (skimage ``resize``: ``ndi.zoom`` order 1, mode "mirror", grid mode) and the labels
(order 0) to ``min(resize_embedding_shape, side)``, then ``regionprops_table(..., ("label", "area", "mean_intensity"))`` - on the
device (csrc/objfeat.hip, ``ops.objfeat_accumulate_batch``): the host builds the per-axis resize tables in double precision, the
kernels sample the labels, sort the pixels by object and sum the bilinearly resampled embedding per object in fp64.  Every unit
(the image, a tile's outer block, a slice, a tile of a slice) of one call runs in batches of bounded workspace (<= 1 GiB); the
tiled / 3-D merge of the reference (areas added, means averaged by area) is the sum over units divided by the total area.

Host fallback: when a resized axis is SHORTER than the 64-pixel embedding grid (a label image smaller than 64 pixels on a side, or a
``resize_embedding_shape`` below 64) skimage anti-aliases with a Gaussian before the zoom; that resample runs on the host with scipy
(as skimage does) and its result goes to the device as a unit with identity tables.

Extensions: segmentations and embeddings may be device tensors (``keep_on_device``); ``project_prediction_to_segmentation`` returns a
device tensor for a device segmentation; tiles missing from a masked tiling (``tiles_in_mask``) are skipped (the reference raises).
Label ids must be non-negative integers below 2^63; predictions must be numeric.
"""
import functools
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops, util
from .tiling import Blocking

GRID = 64                     # the embedding grid of every SAM encoder
CHANNELS = 256
N_FEATURES = 1 + CHANNELS     # area + one mean per channel
WORKSPACE_BYTES = 1 << 30     # device workspace per batch of units
CHUNK = 128                   # sorted pixels per accumulation wave


def nearest_table(side: int, out: int) -> np.ndarray:
    """Source index of every output pixel of ``ndi.zoom(order=0, grid_mode=True)`` from ``side`` to ``out`` pixels (computed in double)."""
    o = np.arange(out, dtype=np.float64)
    return np.floor((o + 0.5) * (np.float64(side) / out) - 0.5 + 0.5).astype(np.int32)


def bilinear_table(side: int, out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(first tap, second tap, weight of the second tap) of ``ndi.zoom(order=1, mode="mirror", grid_mode=True)`` from ``side`` to
    ``out >= side`` pixels: c = (o + 0.5) * side / out - 0.5, taps floor(c) and floor(c) + 1 mirrored into [0, side)."""
    o = np.arange(out, dtype=np.float64)
    c = (o + 0.5) * (np.float64(side) / out) - 0.5
    i0 = np.floor(c)
    w = c - i0
    i0 = i0.astype(np.int64)
    i1 = i0 + 1

    def mirror(i):
        if side == 1:
            return np.zeros_like(i)
        period = 2 * (side - 1)
        i = np.abs(i) % period
        return np.where(i >= side, period - i, i)
    return mirror(i0).astype(np.int32), mirror(i1).astype(np.int32), w


@functools.lru_cache(maxsize=64)
def _unit_tables(side: int, rh: int, rw: int, identity: bool) -> Tuple[np.ndarray, np.ndarray]:
    """int32 [ly, y0, y1, lx, x0, x1] and float32 [wy, wx] of one unit (include/msam_hip.h msam_objfeat_*)."""
    ly, lx = nearest_table(side, rh), nearest_table(side, rw)
    if identity:
        y0 = y1 = np.arange(rh, dtype=np.int32)
        x0 = x1 = np.arange(rw, dtype=np.int32)
        wy, wx = np.zeros(rh), np.zeros(rw)
    else:
        y0, y1, wy = bilinear_table(GRID, rh)
        x0, x1, wx = bilinear_table(GRID, rw)
    return (np.concatenate([ly, y0, y1, lx, x0, x1]).astype(np.int32),
            np.concatenate([wy, wx]).astype(np.float32))


def _resize_embedding_host(emb_chw: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """skimage ``resize(emb.transpose(1, 2, 0), (rh, rw, 256), preserve_range=True)`` for a shrinking axis: Gaussian anti-aliasing
    (sigma = max(0, (64 / R - 1) / 2) per axis, mode "mirror"), zoom order 1, clipped to the input's range.  float32 [rh, rw, 256]."""
    from scipy import ndimage as ndi
    x = np.ascontiguousarray(np.asarray(emb_chw, dtype=np.float32).transpose(1, 2, 0))
    factors = np.divide(x.shape, (rh, rw, CHANNELS))
    sigma = np.maximum(0, (factors - 1) / 2)
    filtered = ndi.gaussian_filter(x, sigma, cval=0, mode="mirror")
    out = ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", cval=0, grid_mode=True)
    return np.clip(out, x.min(), x.max()).astype(np.float32)


def _to_unit_embedding(x, device) -> torch.Tensor:
    """One unit's embedding (tensor / numpy / zarr selection, [1, 256, 64, 64] or [256, 64, 64]) -> fp32 [256, 64, 64] on ``device``."""
    t = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).squeeze()
    if tuple(t.shape) != (CHANNELS, GRID, GRID):
        raise ValueError(f"compute_object_features: an embedding of shape [256, 64, 64] expected, got {tuple(t.shape)}")
    return t


def _labels_to_device(segmentation, device) -> torch.Tensor:
    if torch.is_tensor(segmentation):
        if segmentation.dtype.is_floating_point or segmentation.dtype == torch.bool or segmentation.dtype.is_complex:
            raise TypeError(f"segmentation: integer labels expected, got {segmentation.dtype}")
        t = segmentation.to(device=device).to(torch.int64).contiguous()
    else:
        a = np.asarray(segmentation)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"segmentation: integer labels expected, got {a.dtype}")
        if a.dtype == np.uint64 and a.size and int(a.max()) >= 1 << 63:
            raise ValueError("segmentation: label ids must be below 2^63")
        t = torch.from_numpy(np.ascontiguousarray(a).astype(np.int64, copy=False)).to(device)
    if t.numel() and bool((t < 0).any()):
        raise ValueError("segmentation: label ids must be non-negative")
    return t


def _units(image_embeddings, shape, is_tiled: bool, is_3d: bool):
    """(z, y0, x0, h, w, embedding getter) in the reference's order (_create_seg_and_embed_generator, object_classification.py:60-106)."""
    features = image_embeddings["features"]
    n_slices = shape[0] if is_3d else 1
    if not is_tiled:
        for z in range(n_slices):
            yield z, 0, 0, shape[-2], shape[-1], (lambda z=z: features[z] if is_3d else features[:])
        return
    attrs = features.attrs
    tile_shape, halo = tuple(attrs["tile_shape"]), tuple(attrs["halo"])
    if tuple(attrs["shape"]) != tuple(shape[-2:]):
        raise ValueError(f"compute_object_features: tiled embeddings of shape {tuple(attrs['shape'])} for a segmentation of {tuple(shape)}")
    tiling = Blocking([0, 0], attrs["shape"], tile_shape)
    in_mask = attrs["tiles_in_mask"] if "tiles_in_mask" in attrs else None
    for z in range(n_slices):
        tiles = range(tiling.number_of_blocks)
        if in_mask is not None:
            tiles = sorted(int(t) for t in (in_mask[str(z)] if is_3d else in_mask))
        for tile_id in tiles:
            outer = tiling.get_block_with_halo(tile_id, list(halo)).outer_block
            (y0, x0), (y1, x1) = outer.begin, outer.end
            tile = features[str(tile_id)]
            yield z, y0, x0, y1 - y0, x1 - x0, (lambda tile=tile, z=z: tile[z] if is_3d else tile[:])


def compute_object_features(
    image_embeddings: util.ImageEmbeddings,
    segmentation: np.ndarray,
    resize_embedding_shape: Tuple[int, int] = (256, 256),
    verbose: bool = True,
) -> Tuple[np.ndarray, np.ndarray]:
    """Compute object features based on SAM embeddings (reference object_classification.py:109-193).

    Args:
        image_embeddings: The precomputed image embeddings.
        segmentation: The segmentation for which to compute the features (numpy array or device tensor).
        resize_embedding_shape: Shape for intermediate resizing of the embeddings.
        verbose: Whether to print a progressbar for the computation.

    Returns:
        The segmentation ids (int64).
        The object features [N, 257] (area, 256 means): float64 for 2-D untiled embeddings (only the ids that survive the resizing),
        float32 otherwise (every id of the segmentation; ids that vanish in every unit keep all-zero rows).
    """
    is_tiled = image_embeddings["input_size"] is None
    ndim = segmentation.dim() if torch.is_tensor(segmentation) else np.ndim(segmentation)
    if ndim not in (2, 3):
        raise ValueError(f"compute_object_features: 2-d or 3-d segmentation expected, got {ndim} dimensions")
    is_3d = ndim == 3
    rh, rw = (int(r) for r in resize_embedding_shape)
    if rh < 1 or rw < 1:
        raise ValueError(f"compute_object_features: bad resize_embedding_shape {resize_embedding_shape}")
    device = _lib.require_gpu(segmentation.device if torch.is_tensor(segmentation) and segmentation.is_cuda else None)
    labels = _labels_to_device(segmentation, device)
    shape = tuple(labels.shape)
    ids = torch.unique(labels)
    ids = ids[ids != 0].contiguous()
    n = ids.numel()
    simple = not is_tiled and not is_3d
    out_dtype = torch.float64 if simple else torch.float32
    if n == 0:
        return np.zeros((0,), dtype=np.int64), np.zeros((0, N_FEATURES), dtype=np.float64 if simple else np.float32)
    if n >= 1 << 31:
        raise ValueError("compute_object_features: at most 2^31 - 1 objects")

    units = list(_units(image_embeddings, shape, is_tiled, is_3d))
    sums = torch.zeros((n, CHANNELS), dtype=torch.float64, device=device)
    area_total = torch.zeros((n,), dtype=torch.int64, device=device)
    out = torch.empty((n, N_FEATURES), dtype=out_dtype, device=device)
    plane, width = shape[-2] * shape[-1], shape[-1]

    _, pbar_init, pbar_update, pbar_close = util.handle_pbar(verbose, None, None)
    pbar_init(len(units), "Compute object features")
    batch: List[tuple] = []
    batch_bytes = 0

    def run(batch, last):
        desc = np.zeros((len(batch), ops.OBJFEAT_DESC), dtype=np.int64)
        itabs, ftabs, embs = [], [], []
        it = ft = eo = pix = 0
        for k, (z, y0, x0, h, w, emb_dev, side, urh, urw, host_resized) in enumerate(batch):
            itab, ftab = _unit_tables(side, urh, urw, host_resized)
            eh, ew = (urh, urw) if host_resized else (GRID, GRID)
            desc[k] = (z * plane + y0 * width + x0, width, h, w, eo, ew, urh, urw, it, ft, pix, eh)
            itabs.append(itab)
            ftabs.append(ftab)
            embs.append(emb_dev.reshape(-1))
            it, ft, eo, pix = it + itab.size, ft + ftab.size, eo + eh * ew * CHANNELS, pix + urh * urw
        emb = torch.cat(embs) if len(embs) > 1 else embs[0].contiguous()
        ops.objfeat_accumulate_batch(labels, ids, emb, desc, np.concatenate(itabs), np.concatenate(ftabs), sums, area_total,
                                     out=out if last else None, chunk=CHUNK)

    for i, (z, y0, x0, h, w, get) in enumerate(units):
        side = max(h, w)
        urh, urw = min(rh, side), min(rw, side)
        emb = _to_unit_embedding(get(), device)
        host_resized = urh < GRID or urw < GRID
        if host_resized:
            emb = torch.from_numpy(_resize_embedding_host(emb.cpu().numpy(), urh, urw)).to(device)
        else:
            emb = emb.permute(1, 2, 0).contiguous()          # channel-last: every bilinear tap is 1 KiB contiguous
        unit_bytes = emb.numel() * 4 + urh * urw * 48 + (urh * urw // CHUNK + 1) * 2048
        if batch and (batch_bytes + unit_bytes > WORKSPACE_BYTES or len(batch) >= 4096):
            run(batch, False)
            pbar_update(len(batch))
            batch, batch_bytes = [], 0
        batch.append((z, y0, x0, h, w, emb, side, urh, urw, host_resized))
        batch_bytes += unit_bytes
    run(batch, True)
    pbar_update(len(batch))
    pbar_close()

    seg_ids = ids.cpu().numpy().astype(np.int64)
    features = out.cpu().numpy()
    if simple:
        keep = features[:, 0] > 0
        return seg_ids[keep], features[keep]
    return seg_ids, features


def project_prediction_to_segmentation(
    segmentation: np.ndarray,
    object_prediction: np.ndarray,
    seg_ids: np.ndarray
) -> np.ndarray:
    """Project object level prediction to the corresponding segmentation to obtain a pixel level prediction
    (reference object_classification.py:196-217): every pixel gets the prediction of its id; ids not in ``seg_ids`` (background
    included) get 0.  A device-tensor segmentation gives a device tensor.

    Args:
        segmentation: The segmentation from which the object prediction is derived.
        object_prediction: The object prediction.
        seg_ids: The segmentation ids matching the object prediction.

    Returns:
        The pixel level object prediction, corresponding to a semantic segmentation.
    """
    pred = object_prediction.cpu().numpy() if torch.is_tensor(object_prediction) else np.asarray(object_prediction)
    seg_ids = seg_ids.cpu().numpy() if torch.is_tensor(seg_ids) else np.asarray(seg_ids)
    assert len(pred) == len(seg_ids)
    if pred.dtype.kind not in "biuf":
        raise TypeError(f"project_prediction_to_segmentation: numeric predictions expected, got {pred.dtype}")
    if seg_ids.size and seg_ids.dtype.kind not in "iu":
        raise TypeError(f"project_prediction_to_segmentation: integer seg_ids expected, got {seg_ids.dtype}")
    seg_ids = seg_ids.astype(np.int64).reshape(-1)
    pred = pred.reshape(len(seg_ids))
    order = np.argsort(seg_ids, kind="stable")
    sorted_ids, sorted_pred = seg_ids[order], pred[order]
    last = np.ones(len(sorted_ids), dtype=bool)                # a repeated id takes its last prediction, as a dict built from the pairs
    last[:-1] = sorted_ids[1:] != sorted_ids[:-1]
    sorted_ids, sorted_pred = sorted_ids[last], sorted_pred[last]
    on_device = torch.is_tensor(segmentation) and segmentation.is_cuda
    device = _lib.require_gpu(segmentation.device if on_device else None)
    labels = _labels_to_device(segmentation, device)
    index = ops.objfeat_project(labels, torch.from_numpy(np.ascontiguousarray(sorted_ids)).to(device))
    table = np.concatenate([np.zeros((1,), dtype=pred.dtype), sorted_pred])
    if on_device:
        return torch.from_numpy(table).to(device)[index.to(torch.int64) + 1]
    return table[index.cpu().numpy().astype(np.int64) + 1]


def run_prediction_with_object_classifier(
    images: Sequence[Union[str, os.PathLike, np.ndarray]],
    segmentations: Sequence[Union[str, os.PathLike, np.ndarray]],
    predictor,
    rf_path: Union[str, os.PathLike],
    image_key: Optional[str] = None,
    segmentation_key: Optional[str] = None,
    project_prediction: bool = True,
    ndim: Optional[int] = None,
) -> List[np.ndarray]:
    """Run prediction with a pretrained object classifier on a series of images (reference object_classification.py:224-261).

    Args:
        images: The images, either given as a list of numpy array or filepaths.
        segmentations: The segmentations, either given as a list of numpy array or filepaths.
        predictor: The SAM predictor that computes the embeddings.
        rf_path: The random forest (or any classifier with ``predict``) saved with joblib.
        image_key: The key of the images in container files.
        segmentation_key: The key of the segmentations in container files.
        project_prediction: Whether to project the object predictions onto the segmentation.
        ndim: The dimensionality of the data.

    Returns:
        The predictions.
    """
    from joblib import load
    assert len(images) == len(segmentations)
    rf = load(rf_path)
    predictions = []
    for image, segmentation in zip(images, segmentations):
        if isinstance(image, (str, os.PathLike)):
            image = util.load_image_data(image, key=image_key)
        if isinstance(segmentation, (str, os.PathLike)):
            segmentation = util.load_image_data(segmentation, key=segmentation_key)
        embeddings = util.precompute_image_embeddings(predictor, image, verbose=False, ndim=ndim)
        seg_ids, features = compute_object_features(embeddings, segmentation, verbose=False)
        prediction = rf.predict(features)
        if project_prediction:
            prediction = project_prediction_to_segmentation(segmentation, prediction, seg_ids)
        predictions.append(prediction)
    return predictions
