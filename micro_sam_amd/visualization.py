"""Functionality for visualizing image embeddings (reference micro_sam/visualization.py): the PCA projection of an embedding to an RGB image.

``compute_pca`` restates ``elf.segmentation.embeddings.embedding_pca`` (UNPINNED - elf is not available; restated from its published
source: ``sklearn.decomposition.PCA(n_components).fit_transform`` on the [H * W, C] samples, reshaped to (k, H, W), and with ``as_rgb``
``255 * (x - x.min()) / ptp(x)`` over the whole unit truncated to uint8) on the device (csrc/embedpca.hip, ``ops.pca_moments`` /
``ops.pca_project`` / ``ops.pca_to_rgb``).  A unit - one image, one slice of a stack, one mosaic of a tiled image - stays in the
embedding's own channel-major layout [C, H * W]; all units of a call run as batches of bounded workspace (<= 256 MiB).  Per batch: the
channel means and the centred Gram matrix (two passes, fp32 products on the f32-input MFMA, fp64 sums in a fixed order), the projection
onto the top components with the per-unit minimum and maximum, and the uint8 image.

Host step: the eigen-decomposition.  The [U, C, C] float64 Gram matrices (512 KiB per unit at C = 256, against the 4 MiB embedding) are
copied to the host, one batched ``np.linalg.eigh`` gives the eigenvectors (measured 4.3 ms per 256-channel unit on one core, most of a call: profiles/r07_embedding_pca.md), the top ``k``
get sklearn's sign (``svd_flip(u_based_decision=False)``: the entry of largest magnitude of every component is positive) and go back
as float32 [U, k, C] (3 KiB per unit).  The embedding itself is never copied to the host.

Tiled embeddings: the reference's mosaic - per tile the aspect crop and the inner block with bounds ``int(np.round(coord * scale))``
(numpy's round half to even), the tiles of a row resized to the row's largest height and the rows to the largest width - is assembled with
torch indexing on the device; the resize (skimage ``resize``, enlarging only) is restated as ``ndi.zoom(order=1, mode="mirror",
grid_mode=True)`` through ``object_classification.bilinear_table``, UNPINNED against the absent skimage as in that module.

Extensions: embeddings may be device tensors (``precompute_image_embeddings(..., keep_on_device=True)``), the result is then a device
tensor; numpy (and zarr) input gives numpy output.  Differences: a unit whose projection is constant (``ptp == 0``) gives an all-zero uint8
image (the reference divides by zero); ``n_components`` is limited to ``min(8, H * W, C)`` and ``C`` to 256; non-floating embeddings raise
``TypeError``; embeddings are read as float32; tilings with missing tiles (``tiles_in_mask``) raise ``ValueError``.
"""
from typing import Tuple

import numpy as np
import torch

from . import _lib, ops
from .object_classification import bilinear_table
from .tiling import Blocking
from .util import ImageEmbeddings

WORKSPACE_BYTES = 1 << 28     # device workspace per batch of units
MAX_COMPONENTS = ops.PCA_MAX_COMPONENTS
MAX_CHANNELS = ops.PCA_MAX_CHANNELS


#
# PCA visualization for the image embeddings
#

def _load(x):
    """A tensor or numpy array from a tensor, numpy array, zarr array or ``TileArray``."""
    if not (torch.is_tensor(x) or isinstance(x, np.ndarray)):
        x = x[:]
    return x.detach() if torch.is_tensor(x) else np.asarray(x)


def _check_floating(x) -> None:
    floating = x.dtype.is_floating_point if torch.is_tensor(x) else np.issubdtype(x.dtype, np.floating)
    if not floating:
        raise TypeError(f"compute_pca: floating-point embeddings expected, got {x.dtype}")


def _components(gram: torch.Tensor, n_components: int) -> torch.Tensor:
    """The host step: float32 [U, k, C] principal axes of the double [U, C, C] Gram matrices, in sklearn's order and sign."""
    _, vec = np.linalg.eigh(gram.cpu().numpy())                          # ascending eigenvalues, eigenvectors in columns
    comp = np.ascontiguousarray(vec[:, :, ::-1][:, :, :n_components].transpose(0, 2, 1))
    largest = np.take_along_axis(comp, np.abs(comp).argmax(axis=2)[:, :, None], axis=2)
    comp *= np.where(largest < 0, -1.0, 1.0)
    return torch.from_numpy(comp.astype(np.float32)).to(gram.device)


def _pca_units(x: torch.Tensor, n_components: int, as_rgb: bool) -> torch.Tensor:
    """x float32 [U, C, N] on the device -> uint8 [U, N, 3] (``as_rgb``) or float32 [U, N, k]; every unit on its own."""
    n_units, channels, positions = x.shape
    per_unit = ops.pca_moments_workspace_bytes(1, channels, positions)
    group = max(1, min(n_units, WORKSPACE_BYTES // max(per_unit, 1), ops.PCA_MAX_UNITS))
    outs = []
    for u0 in range(0, n_units, group):
        xs = x[u0:u0 + group]
        mean, gram = ops.pca_moments(xs)
        proj, minmax = ops.pca_project(xs, _components(gram, n_components), mean)
        outs.append(ops.pca_to_rgb(proj, minmax) if as_rgb else proj.permute(0, 2, 1))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def compute_pca(embeddings: np.ndarray, n_components: int = 3, as_rgb: bool = True) -> np.ndarray:
    """Compute the pca projection of the embeddings to visualize them as RGB image.

    Args:
        embeddings: The embeddings. For example predicted by the SAM image encoder: [1, C, H, W], or [Z, 1, C, H, W] - every slice is
            then fitted and normalised on its own.  A numpy array or a tensor (a device tensor stays on the device).
        n_components: The number of PCA components to use for dimensionality reduction.
        as_rgb: Whether to normalize the projected embeddings so that they can be displated as rgb.

    Returns:
        PCA of the embeddings, mapped to the pixels: (H, W, k) or (Z, H, W, k); uint8 with ``as_rgb``, else float32.
    """
    emb = _load(embeddings)
    if emb.ndim not in (4, 5):
        raise ValueError(f"Expect input of ndim 4 or 5, got {emb.ndim}")
    _check_floating(emb)
    if as_rgb and n_components != 3:
        raise ValueError(f"compute_pca: as_rgb needs n_components == 3, got {n_components}")
    shape = tuple(int(s) for s in emb.shape)
    if shape[-4] != 1 or (emb.ndim == 5 and shape[0] < 1):
        raise ValueError(f"compute_pca: embeddings of shape [1, C, H, W] or [Z >= 1, 1, C, H, W] expected, got {list(shape)}")
    channels, height, width = shape[-3:]
    n_units = shape[0] if emb.ndim == 5 else 1
    if channels < 1 or height < 1 or width < 1 or channels > MAX_CHANNELS:
        raise ValueError(f"compute_pca: 1 to {MAX_CHANNELS} channels and a non-empty grid expected, got {list(shape)}")
    n_components = int(n_components)
    if not 1 <= n_components <= min(MAX_COMPONENTS, height * width, channels):
        raise ValueError(f"compute_pca: n_components must lie in [1, min({MAX_COMPONENTS}, H * W, C)], got {n_components} for {list(shape)}")
    is_tensor = torch.is_tensor(emb)
    home = emb.device if is_tensor else None
    device = _lib.require_gpu(home if is_tensor and emb.is_cuda else None)
    t = emb if is_tensor else torch.from_numpy(np.ascontiguousarray(emb))
    x = t.to(device=device, dtype=torch.float32).reshape(n_units, channels, height * width).contiguous()
    vis = _pca_units(x, n_components, as_rgb).reshape(n_units, height, width, n_components)
    if emb.ndim == 4:
        vis = vis[0]
    if not is_tensor:
        return vis.cpu().numpy()
    return vis.to(home)


def _get_crop(embed_shape, shape):
    """Index of the part of an (h, w, ...) grid that an image of ``shape``, padded to a square at its lower / right side, covers."""
    rows, cols = shape[0], shape[1]
    if rows > cols:
        return (slice(None), slice(None, int(float(cols / rows) * embed_shape[1])))
    if cols > rows:
        return (slice(None, int(float(rows / cols) * embed_shape[0])), slice(None))
    return (slice(None), slice(None), slice(None))


def _project_embeddings(embeddings, shape, apply_crop=True, n_components=3, as_rgb=True):
    """PCA over the full grid (padding included), the crop to the image's aspect afterwards; scale = image shape / result shape."""
    if embeddings.ndim != len(shape) + 2:
        raise ValueError(f"embeddings of shape {tuple(embeddings.shape)} do not belong to data of shape {tuple(shape)}")
    if len(shape) not in (2, 3):
        raise ValueError(f"Expect 2d or 3d data, got {len(shape)}")
    embedding_vis = compute_pca(embeddings, n_components=n_components, as_rgb=as_rgb)
    if apply_crop:
        lead = (slice(None),) * (len(shape) - 2)
        embedding_vis = embedding_vis[lead + _get_crop(embedding_vis.shape[len(lead):], shape[len(lead):])]
    scale = tuple(float(size) / vis_size for size, vis_size in zip(shape, embedding_vis.shape))
    return embedding_vis, scale


def _project_embeddings_to_tile(tile, tile_embeds):
    """The part of a tile's embedding ([1, C, h, w] or [Z, 1, C, h, w]) that belongs to the tile's inner block: the aspect crop of the
    outer block, then the inner block with bounds rounded half to even (``np.round``) in embedding coordinates."""
    outer, inner = tile.outer_block, tile.inner_block_local
    outer_shape = (outer.end[0] - outer.begin[0], outer.end[1] - outer.begin[1])
    lead = (slice(None),) * (tile_embeds.ndim - 2)
    cropped = tile_embeds[lead + _get_crop(tile_embeds.shape[-2:], outer_shape)[:2]]
    bounds = []
    for axis in range(2):
        scale = cropped.shape[-2 + axis] / float(outer_shape[axis])
        bounds.append(slice(int(np.round(inner.begin[axis] * scale)), int(np.round(inner.end[axis] * scale))))
    return cropped[lead + tuple(bounds)]


def _resize_axis(t: torch.Tensor, axis: int, length: int) -> torch.Tensor:
    """``ndi.zoom(order=1, mode="mirror", grid_mode=True)`` of one axis to ``length >= t.shape[axis]``: two taps per output index,
    combined in double and rounded to the tensor's type."""
    side = int(t.shape[axis])
    if side == length:
        return t
    if length < side:
        raise ValueError(f"_resize_and_cocatenate: only enlarging resizes are supported, got {side} -> {length}")
    i0, i1, w = bilinear_table(side, length)
    wshape = [1] * t.ndim
    wshape[axis] = length
    wt = torch.from_numpy(w).to(t.device).reshape(wshape)
    a = t.index_select(axis, torch.from_numpy(i0.astype(np.int64)).to(t.device)).double()
    b = t.index_select(axis, torch.from_numpy(i1.astype(np.int64)).to(t.device)).double()
    return ((1.0 - wt) * a + wt * b).to(t.dtype)


def _resize_and_cocatenate(arrays, axis):
    """Concatenate along ``axis`` (-1 or -2) after resizing the other of the two axes to its largest length among ``arrays``."""
    assert axis in (-1, -2)
    resize_axis = -1 if axis == -2 else -2
    as_numpy = not torch.is_tensor(arrays[0])
    tensors = [torch.from_numpy(np.ascontiguousarray(arr)) if as_numpy else arr for arr in arrays]
    resize_len = max([int(arr.shape[resize_axis]) for arr in tensors])
    out = torch.cat([_resize_axis(arr, arr.ndim + resize_axis, resize_len) for arr in tensors], dim=axis)
    return out.numpy() if as_numpy else out


def _project_tiled_embeddings(image_embeddings, n_components, as_rgb):
    features = image_embeddings["features"]
    tile_shape, halo, shape = features.attrs["tile_shape"], features.attrs["halo"], features.attrs["shape"]
    tile_shape, halo, shape = tuple(tile_shape), tuple(halo), tuple(shape)
    tiling = Blocking([0, 0], shape, tile_shape)

    tile_grid = tiling.blocks_per_axis

    embeds = {
        i: {j: None for j in range(tile_grid[1])} for i in range(tile_grid[0])
    }

    is_tensor, home, device, ndim = None, None, None, None
    for tile_id in range(tiling.number_of_blocks):
        if str(tile_id) not in features:
            raise ValueError(f"project_embeddings_for_visualization: tile {tile_id} is missing from the tiled embeddings (a masked tiling?)")
        tile_embeds = _load(features[str(tile_id)])
        assert tile_embeds.ndim in (4, 5)
        _check_floating(tile_embeds)
        if device is None:                                               # the first tile decides where the mosaic lives and what comes back
            is_tensor, ndim = torch.is_tensor(tile_embeds), tile_embeds.ndim
            home = tile_embeds.device if is_tensor else None
            device = _lib.require_gpu(home if is_tensor and tile_embeds.is_cuda else None)
        if not torch.is_tensor(tile_embeds):
            tile_embeds = torch.from_numpy(np.ascontiguousarray(tile_embeds))
        tile_embeds = tile_embeds.to(device=device, dtype=torch.float32)

        # extract the embeddings corresponding to the inner tile
        tile = tiling.get_block_with_halo(tile_id, list(halo))
        i, j = tiling._coords(tile_id)
        embeds[i][j] = _project_embeddings_to_tile(tile, tile_embeds)

    embeds = _resize_and_cocatenate(
        [
            _resize_and_cocatenate(
                [embeds[i][j] for j in range(tile_grid[1])], axis=-1
            )
            for i in range(tile_grid[0])
        ], axis=-2
    )

    if ndim == 5:
        shape = (int(embeds.shape[0]),) + tuple(shape)
    embedding_vis, scale = _project_embeddings(
        embeds, shape, n_components=n_components, as_rgb=as_rgb, apply_crop=False
    )
    if not is_tensor:
        embedding_vis = embedding_vis.cpu().numpy()
    elif embedding_vis.device != home:
        embedding_vis = embedding_vis.to(home)
    return embedding_vis, scale


def project_embeddings_for_visualization(
    image_embeddings: ImageEmbeddings, n_components: int = 3, as_rgb: bool = True,
) -> Tuple[np.ndarray, Tuple[float, ...]]:
    """Project image embeddings to pixel-wise PCA.

    Args:
        image_embeddings: The image embeddings.
        n_components: The number of PCA components to use for dimensionality reduction.
        as_rgb: Whether to normalize the projected embeddings so that they can be displated as rgb.

    Returns:
        The PCA of the embeddings (a device tensor for device-resident embeddings, else a numpy array).
        The scale factor for resizing to the original image size.
    """
    if image_embeddings["input_size"] is None:                           # tiled embeddings carry their sizes per tile
        return _project_tiled_embeddings(image_embeddings, n_components, as_rgb)
    embeddings = _load(image_embeddings["features"])
    shape = tuple(image_embeddings["original_size"])
    if embeddings.ndim == 5:
        shape = (int(embeddings.shape[0]),) + shape
    return _project_embeddings(embeddings, shape, n_components=n_components, as_rgb=as_rgb)
