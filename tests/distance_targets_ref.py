"""Test helper: a numpy / scipy restatement of torch_em's ``PerObjectDistanceTransform`` (the training targets of the convolutional
decoder) in its PER-OBJECT CROP form, and the label images the host and the device tests share.  TEST INFRASTRUCTURE.

torch_em is neither vendored in the reference nor installed here: this follows its published source and is UNPINNED.
Per object, as there: crop the object's bounding box, take the distance transform of the image's inner boundaries
(``skimage.segmentation.find_boundaries(labels, mode="inner")``: only neighbours inside the image count) CROPPED to that box, mask it to
the object, normalise by its maximum and invert; the centre is the rounded centroid (``np.round``: half to even), replaced by the arg-max
of the masked boundary distances when it lies outside the object; the distances to the centre are normalised by their maximum over the
crop.  csrc/labelprops.hip computes one distance transform for the whole image instead - that shortcut is what the tests check.

Where this file follows the contract of ``msam_distance_targets`` rather than torch_em's lines: the arg-max runs over the object's
pixels only (torch_em zeroes the distances outside the object, so an object without an interior pixel would get the crop's first pixel),
and an image without any boundary pixel has ``dmax2 = 0`` and a boundary channel of 1.
"""
import numpy as np
from scipy import ndimage

import labelprops_ref as LR

EPS = 1e-7


def find_boundaries_inner(labels: np.ndarray) -> np.ndarray:
    """bool [H, W]: foreground pixels with a 4-neighbour inside the image that holds another value."""
    lab = np.asarray(labels).astype(np.int64)
    b = np.zeros(lab.shape, bool)
    b[1:, :] |= lab[1:, :] != lab[:-1, :]
    b[:-1, :] |= lab[:-1, :] != lab[1:, :]
    b[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    b[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    return b & (lab != 0)


def distance_targets(labels: np.ndarray, n: int = None, fill: float = 1.0, correct_centers: bool = True):
    """labels [H, W] -> dict: out float64 [3, H, W] (foreground, centre distance, boundary distance), center int64 [N, 2], dmax2 int64 [N],
    bbox int64 [N, 4].  Objects are 1..n (n = the maximum by default); every other value is background.  A label the image does not hold:
    bbox 0, center -1, dmax2 0."""
    lab = np.asarray(labels).astype(np.int64)
    if n is None:
        n = int(max(lab.max(), 0))
    lab = np.where((lab >= 1) & (lab <= n), lab, 0)
    h, w = lab.shape
    out = np.stack([(lab != 0).astype(np.float64), np.full((h, w), float(fill)), np.full((h, w), float(fill))])
    center, dmax2, bbox = np.full((n, 2), -1, np.int64), np.zeros(n, np.int64), np.zeros((n, 4), np.int64)
    boundaries = find_boundaries_inner(lab)
    for k, sl in enumerate(ndimage.find_objects(lab.astype(np.int32), max_label=n)):
        if sl is None:
            continue
        y0, x0 = sl[0].start, sl[1].start
        mask = lab[sl] == k + 1
        ys, xs = np.nonzero(mask)
        c = (int(np.round((ys.sum() + y0 * len(ys)) / len(ys))) - y0, int(np.round((xs.sum() + x0 * len(xs)) / len(xs))) - x0)
        crop_b = boundaries[sl]
        if crop_b.any():
            d = ndimage.distance_transform_edt(~crop_b)
            d2 = np.rint(d * d).astype(np.int64)
        else:
            d2 = np.zeros(mask.shape, np.int64)                                      # no boundary pixel anywhere: the contract's case
        masked = np.where(mask, d2, -1)
        dm = int(masked.max())
        if correct_centers and not mask[c]:
            c = np.unravel_index(int(np.argmax(masked)), masked.shape)              # the first in raster order
        yy, xx = np.mgrid[:mask.shape[0], :mask.shape[1]]
        dist = np.sqrt(((yy - c[0]) ** 2 + (xx - c[1]) ** 2).astype(np.float64))
        dist = dist / (dist.max() + EPS)                                             # over the crop, before masking
        bd = 1.0 - np.sqrt(d2.astype(np.float64)) / (np.sqrt(float(dm)) + EPS)
        out[1][sl][mask] = dist[mask]
        out[2][sl][mask] = bd[mask]
        center[k] = (c[0] + y0, c[1] + x0)
        dmax2[k] = dm
        bbox[k] = (y0, x0, sl[0].stop, sl[1].stop)
    return {"out": out, "center": center, "dmax2": dmax2, "bbox": bbox}


def relabel_consecutive(seg: np.ndarray) -> np.ndarray:
    """Positive values -> 1..N in ascending order, everything else -> 0."""
    seg = np.asarray(seg).astype(np.int64)
    ids = np.unique(seg)
    ids = ids[ids > 0]
    out = np.searchsorted(ids, seg) + 1
    return np.where(seg > 0, out, 0).astype(np.int32)


def label_components(seg: np.ndarray) -> np.ndarray:
    """``skimage.measure.label`` defaults restated with scipy.ndimage: components of equal non-zero value under 8-connectivity, numbered
    by their first pixel in raster order."""
    seg = np.asarray(seg)
    out = np.zeros(seg.shape, np.int64)
    firsts = []
    for v in np.unique(seg):
        if v == 0:
            continue
        comp, k = ndimage.label(seg == v, structure=np.ones((3, 3)))
        for c in range(1, k + 1):
            m = comp == c
            firsts.append((int(np.flatnonzero(m)[0]), m))
    for i, (_, m) in enumerate(sorted(firsts, key=lambda t: t[0]), start=1):
        out[m] = i
    return out.astype(np.int32)


def transform(seg: np.ndarray, apply_label=True, min_size=0, fill=1.0, correct_centers=True):
    """The whole transform with all four channels: [instances, foreground, centre, boundary] float64, and the label image used."""
    lab = label_components(seg) if apply_label else np.asarray(seg).astype(np.int64)
    if min_size > 0:
        ids, sizes = np.unique(lab, return_counts=True)
        lab = np.where(np.isin(lab, ids[sizes < min_size]), 0, lab)
    lab = relabel_consecutive(lab)
    t = distance_targets(lab, fill=fill, correct_centers=correct_centers)
    return np.concatenate([lab[None].astype(np.float64), t["out"]]), lab


def cases():
    """name -> (label image int32 [H, W], N): objects are 1..N."""
    out = {}
    for name, (seg, _) in LR.cases().items():
        lab = relabel_consecutive(seg)
        out[name] = (lab, int(lab.max()))
    stray = relabel_consecutive(LR.voronoi(33, 65, 9, 1))
    n = int(stray.max())
    stray[2, 3] = n + 5; stray[20:23, 40:44] = -4; stray[32, 64] = 2 ** 31 - 1; stray[0, 0] = -2 ** 31
    out["out_of_range"] = (stray, n)
    absent = relabel_consecutive(LR.voronoi(33, 65, 9, 1))
    out["absent_last"] = (absent, int(absent.max()) + 2)                             # two labels the image does not hold
    return out


def two_piece() -> np.ndarray:
    """One value in two pieces (plus a diagonal bridge that 8-connectivity joins), for ``apply_label``."""
    seg = np.zeros((24, 31), np.int32)
    seg[2:9, 3:12] = 5
    seg[14:22, 15:28] = 5                                                            # the second piece of value 5
    seg[9, 12] = 5                                                                   # touches the first piece by a corner only: the same component
    seg[3:10, 20:29] = 2
    return seg


def min_size_case() -> np.ndarray:
    """Three objects of which the middle id is the small one."""
    seg = np.zeros((20, 40), np.int32)
    seg[1:9, 1:12] = 1
    seg[10:13, 15:18] = 2                                                            # 9 pixels
    seg[5:18, 22:38] = 3
    return seg
