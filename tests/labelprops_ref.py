"""Test helper: a numpy / scipy restatement of what csrc/labelprops.hip computes, and the label images the host and the device tests share.
TEST INFRASTRUCTURE.

* ``inner_boundaries``: ``skimage.segmentation.find_boundaries(np.pad(seg, 1), mode="inner")`` restated as minimum != maximum over the
  4-cross of the zero-padded image, restricted to the foreground (scikit-image is not available here: unpinned).
* ``edt_squared``: ``scipy.ndimage.distance_transform_edt`` squared and rounded to integers (float64 holds the square root of an integer
  below 2^31 closely enough that squaring and rounding gives the integer back); ``edt_squared_brute``: the nearest zero by exhaustive
  search, a second opinion for sides <= 48.
* ``label_props``: area, bbox (exclusive ends), coordinate sums, centroid, and the "v" centre by the reference's own lines
  (micro_sam/util.py:1314-1326): the float distance field of the padded boundaries, ``np.where(prop.image, region, -1.0)``, ``argmax``.
"""
import numpy as np
from scipy import ndimage

INT32_MAX = 2 ** 31 - 1


def inner_boundaries(seg: np.ndarray) -> np.ndarray:
    """bool [H + 2, W + 2]: the inner boundaries of ``np.pad(seg, 1)``."""
    p = np.pad(np.asarray(seg).astype(np.int64), 1)
    q = np.pad(p, 1)                                     # (what lies outside the padded image never matters: its rim is background)
    cross = np.stack([q[1:-1, 1:-1], q[:-2, 1:-1], q[2:, 1:-1], q[1:-1, :-2], q[1:-1, 2:]])
    return (cross.min(axis=0) != cross.max(axis=0)) & (p != 0)


def edt_squared(mask: np.ndarray) -> np.ndarray:
    """int64 [H, W]: squared distance to the nearest zero pixel; INT32_MAX everywhere when there is none."""
    mask = np.asarray(mask) != 0
    if mask.all():
        return np.full(mask.shape, INT32_MAX, np.int64)
    d = ndimage.distance_transform_edt(mask)
    return np.rint(d * d).astype(np.int64)


def edt_squared_brute(mask: np.ndarray) -> np.ndarray:
    mask = np.asarray(mask) != 0
    assert max(mask.shape) <= 48
    zy, zx = np.nonzero(~mask)
    if len(zy) == 0:
        return np.full(mask.shape, INT32_MAX, np.int64)
    yy, xx = np.mgrid[:mask.shape[0], :mask.shape[1]]
    return ((yy[..., None] - zy) ** 2 + (xx[..., None] - zx) ** 2).min(axis=-1).astype(np.int64)


def label_props(seg: np.ndarray, ids=None):
    """-> dict: ids int64 [N], area int64 [N], bbox int64 [N, 4], coord_sum int64 [N, 2], centroid float64 [N, 2], center int64 [N, 2].
    An id the image does not hold: area 0, bbox 0, center -1 (the library's convention), centroid nan."""
    seg = np.asarray(seg).astype(np.int64)
    if ids is None:
        ids = np.unique(seg)
        ids = ids[ids > 0]
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    out = {"ids": ids, "area": np.zeros(n, np.int64), "bbox": np.zeros((n, 4), np.int64), "coord_sum": np.zeros((n, 2), np.int64),
           "centroid": np.full((n, 2), np.nan), "center": np.full((n, 2), -1, np.int64)}
    if n == 0:
        return out
    distances = ndimage.distance_transform_edt(inner_boundaries(seg) == 0)          # of the padded image (reference :1314-1316)
    fg = np.where(seg > 0, seg, 0)
    compact = np.searchsorted(ids, fg)
    compact = np.where((fg > 0) & (ids[np.minimum(compact, n - 1)] == fg), np.minimum(compact, n - 1) + 1, 0).astype(np.int32)
    for k, sl in enumerate(ndimage.find_objects(compact, max_label=n)):
        if sl is None:
            continue
        image = compact[sl] == k + 1                                                # regionprops: prop.image
        bbox = (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)                   # prop.bbox
        ys, xs = np.nonzero(image)
        out["area"][k] = len(ys)
        out["bbox"][k] = bbox
        out["coord_sum"][k] = (ys.sum() + bbox[0] * len(ys), xs.sum() + bbox[1] * len(ys))
        out["centroid"][k] = ((ys + bbox[0]).mean(), (xs + bbox[1]).mean())        # prop.centroid
        region = distances[bbox[0] + 1:bbox[2] + 1, bbox[1] + 1:bbox[3] + 1]        # reference :1323-1326
        masked = np.where(image, region, -1.0)
        local = np.unravel_index(int(np.argmax(masked)), masked.shape)
        out["center"][k] = (local[0] + bbox[0], local[1] + bbox[1])
    return out


# ---------------------------------------------------------------------------------------------------------------- label images

def voronoi(h: int, w: int, n: int, seed: int, band=True) -> np.ndarray:
    """Seeded Voronoi cells with ids 1..n (in seed order), a background band across the image and every seventh cell removed."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((h, w), np.int32)
    ys, xs = rng.integers(0, h, n), rng.integers(0, w, n)
    pts[ys, xs] = np.arange(1, n + 1)
    idx = ndimage.distance_transform_edt(pts == 0, return_distances=False, return_indices=True)
    seg = pts[idx[0], idx[1]]
    if band:
        seg[int(h * 0.4):int(h * 0.4) + max(h // 10, 1)] = 0
        seg[seg % 7 == 3] = 0
    return seg


def ring(size: int = 41, label: int = 2) -> np.ndarray:
    yy, xx = np.mgrid[:size, :size]
    r2 = (yy - size // 2) ** 2 + (xx - size // 2) ** 2
    return np.where((r2 <= (size // 2 - 2) ** 2) & (r2 >= (size // 4) ** 2), label, 0).astype(np.int32)


def letter_c(size: int = 41, label: int = 9) -> np.ndarray:
    seg = ring(size, label)
    seg[size // 2 - 4:size // 2 + 5, size // 2:] = 0                               # open to the right: the centroid stays in the hole
    return seg


def bar() -> np.ndarray:
    seg = np.zeros((9, 30), np.int32)
    seg[3:5, 4:26] = 4                                                              # 2 pixels wide: every pixel is a boundary
    seg[6:9, 0:30] = 6                                                              # 3 wide, touching three borders: a row of ties
    return seg


def cases():
    """name -> (label image int32 [H, W], ids or None)."""
    rng = np.random.default_rng(7)
    out = {
        "1x1": (np.array([[3]], np.int32), None),
        "1x7": (np.array([[1, 1, 0, 2, 2, 2, 5]], np.int32), None),
        "7x1": (np.array([[1, 1, 0, 2, 2, 2, 5]], np.int32).T.copy(), None),
        "33x65": (voronoi(33, 65, 9, 1), None),
        "64x64": (voronoi(64, 64, 12, 2), None),
        "130x257": (voronoi(130, 257, 20, 3), None),
        "full": (np.full((33, 65), 7, np.int32), None),
        "ring": (ring(), None),
        "c": (letter_c(), None),
        "bar": (bar(), None),
        "checkerboard": ((np.arange(1, 64 * 64 + 1).reshape(64, 64) * (np.add.outer(np.arange(64), np.arange(64)) % 2 == 0)).astype(np.int32), None),
    }
    single = np.zeros((20, 23), np.int32)
    ys, xs = rng.integers(0, 20, 15), rng.integers(0, 23, 15)
    single[ys, xs] = np.arange(1, 16)
    out["single_pixels"] = (single, None)
    big = np.zeros((40, 70), np.int32)
    big[2:12, 3:30] = 5; big[12:30, 3:20] = 1000; big[5:38, 40:69] = 70000; big[20:25, 45:50] = 0
    out["big_ids"] = (big, None)
    out["subset_and_absent"] = (voronoi(33, 65, 9, 1), np.array([2, 4, 8, 400], np.int32))      # 400 is not in the image
    assert len(np.unique(out["checkerboard"][0])) == 2049
    return out


def edt_masks():
    """name -> mask (uint8) for edt_squared alone."""
    rng = np.random.default_rng(11)
    corner = np.ones((40, 45), np.uint8); corner[0, 0] = 0
    columns = (rng.random((37, 41)) > 0.15).astype(np.uint8); columns[:, [0, 5, 6, 40]] = 1       # columns without any zero
    row = np.ones((3, 257), np.uint8); row[1, 256] = 0                                             # the scan leaves the staged part
    wide = np.ones((5, 700), np.uint8); wide[2, 3] = 0; wide[4, 690] = 0
    noise = (rng.random((48, 47)) > 0.05).astype(np.uint8)
    tall = np.ones((100, 9), np.uint8)                                                              # four segments of the column pass
    for y, x in ((0, 0), (99, 1), (40, 2), (31, 3), (32, 4), (63, 5), (64, 5), (5, 7), (95, 7)):
        tall[y, x] = 0
    return {"corner": corner, "columns": columns, "no_zero": np.ones((9, 13), np.uint8), "row257": row, "wide": wide, "noise": noise, "tall": tall,
            "all_zero": np.zeros((4, 6), np.uint8), "1x1": np.ones((1, 1), np.uint8)}
