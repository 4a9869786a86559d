"""CPU restatement of the reference's micro_sam/object_classification.py for the tests (the product never imports it).

skimage's ``resize`` (0.2x, ``preserve_range=True``) is ``scipy.ndimage.zoom(..., mode="mirror", grid_mode=True)`` after a Gaussian
prefilter when an axis shrinks (order 1) and a clip to the input's range; ``regionprops_table(label, area, mean_intensity)`` is a
per-label pixel count and an fp64 ``np.bincount`` sum of every channel.  The tiled / 3-D merge is the reference's literal ``visited`` loop.
"""
import numpy as np
from scipy import ndimage as ndi


def sk_resize(image: np.ndarray, output_shape, order: int) -> np.ndarray:
    """skimage.transform.resize(image, output_shape, order, preserve_range=True, anti_aliasing=None (order 1) / False (order 0))."""
    output_shape = tuple(output_shape)
    factors = np.divide(image.shape, output_shape)
    if order == 0:
        return ndi.zoom(image, [1 / f for f in factors], order=0, mode="mirror", cval=0, grid_mode=True)
    image = image.astype(np.float32, copy=False)
    filtered = image
    if any(x < y for x, y in zip(output_shape, image.shape)):
        sigma = np.maximum(0, (factors - 1) / 2)
        filtered = ndi.gaussian_filter(image, sigma, cval=0, mode="mirror")
    out = ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", cval=0, grid_mode=True)
    return np.clip(out, image.min(), image.max())


def compute_object_features_impl(embeddings: np.ndarray, segmentation: np.ndarray, resize_embedding_shape):
    """object_classification.py:20-57 -> (ids int64, features float64 [N, 257])."""
    embeddings = np.asarray(embeddings, dtype=np.float32).transpose(1, 2, 0)
    h, w = segmentation.shape
    s = max(h, w)
    seg = np.pad(segmentation, ((0, s - h), (0, s - w)))
    resize_shape = tuple(min(r, s) for r in resize_embedding_shape) + (embeddings.shape[-1],)
    emb = sk_resize(embeddings, resize_shape, order=1).astype(np.float32)
    seg_r = sk_resize(seg, emb.shape[:2], order=0).astype(segmentation.dtype)
    flat = seg_r.reshape(-1).astype(np.int64)
    ids = np.unique(flat)
    ids = ids[ids > 0]
    idx = np.searchsorted(ids, flat)
    fg = flat > 0
    area = np.bincount(idx[fg], minlength=len(ids)).astype(np.float64)
    e = emb.reshape(-1, emb.shape[-1])[fg].astype(np.float64)
    sums = np.stack([np.bincount(idx[fg], weights=e[:, c], minlength=len(ids)) for c in range(e.shape[1])], axis=1)
    feats = np.concatenate([area[:, None], sums / np.maximum(area, 1)[:, None]], axis=1) if len(ids) else np.zeros((0, 257))
    return ids.astype(np.int64), feats


def _units(segmentation, features, is_tiled, is_3d, tile_blocks=None):
    """(seg, embedding) per unit in the reference's order; ``tile_blocks``: [(tile_id, (y0, x0, y1, x1))] of the tiling."""
    slices = range(segmentation.shape[0]) if is_3d else [None]
    for z in slices:
        seg_z = segmentation if z is None else segmentation[z]
        if not is_tiled:
            yield seg_z, np.asarray(features if z is None else features[z]).squeeze()
            continue
        for tile_id, (y0, x0, y1, x1) in tile_blocks:
            emb = features[str(tile_id)]
            emb = emb[:] if z is None else emb[z]
            yield seg_z[y0:y1, x0:x1], np.asarray(emb.cpu() if hasattr(emb, "cpu") else emb).squeeze()


def compute_object_features(features, segmentation, is_tiled=False, tile_blocks=None, resize_embedding_shape=(256, 256)):
    """object_classification.py:109-193 with the embeddings as host arrays (``features`` as in image_embeddings["features"])."""
    is_3d = segmentation.ndim == 3
    if not is_tiled and not is_3d:
        return compute_object_features_impl(np.asarray(features).squeeze(), segmentation, resize_embedding_shape)
    seg_ids = np.unique(segmentation).tolist()
    if seg_ids and seg_ids[0] == 0:
        seg_ids = seg_ids[1:]
    visited = {seg_id: False for seg_id in seg_ids}
    features_out = np.zeros((len(seg_ids), 257), dtype="float32")
    for seg, embeds in _units(segmentation, features, is_tiled, is_3d, tile_blocks):
        this_seg_ids, this_features = compute_object_features_impl(embeds, seg, resize_embedding_shape)
        this_seg_ids = this_seg_ids.tolist()
        new_idx = np.array([seg_ids.index(i) for i in this_seg_ids if not visited[i]], dtype="int")
        visited_idx = np.array([seg_ids.index(i) for i in this_seg_ids if visited[i]], dtype="int")
        this_new_idx = np.array([this_seg_ids.index(i) for i in this_seg_ids if not visited[i]], dtype="int")
        this_visited_idx = np.array([this_seg_ids.index(i) for i in this_seg_ids if visited[i]], dtype="int")
        features_out[new_idx] = this_features[this_new_idx]
        if len(visited_idx) > 0:
            prev_size = features_out[visited_idx, 0:1]
            this_size = this_features[this_visited_idx, 0:1]
            features_out[visited_idx, 0] += this_features[this_visited_idx, 0]
            features_out[visited_idx, 1:] = (prev_size * features_out[visited_idx, 1:] + this_size * this_features[this_visited_idx, 1:]) / (
                prev_size + this_size)
        visited.update({i: True for i in this_seg_ids})
    return np.array(seg_ids, dtype=np.int64), features_out


def project_prediction_to_segmentation(segmentation, object_prediction, seg_ids):
    """object_classification.py:196-217 as a Python dict lookup."""
    prediction = {int(i): p for i, p in zip(seg_ids, object_prediction)}
    flat = np.asarray(segmentation).reshape(-1)
    return np.array([prediction.get(int(v), 0) for v in flat], dtype=np.asarray(object_prediction).dtype).reshape(np.shape(segmentation))
