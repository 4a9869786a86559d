"""Shared inputs of tests/test_tiled_merge_host.py and tests/test_gpu_tiled_merge.py: tile-local records with ragged geometry, their record
table (csrc/tilemerge.hip) built with numpy, and the numpy references of the two kernels.  TEST INFRASTRUCTURE.

The generator is ``_tiled_records`` of tests/test_prompt_derivation_host.py with tiles of 150 x 200 (wpc = 5, 22 tail bits), tile origins
whose y differ by 110, 100 and 10 rows - never a multiple of 32, so the bit masks of two tiles are misaligned - and radii up to 44, so that
windows span three and more word rows."""
import numpy as np

IMAGE, TILE = (300, 420), (150, 200)
ORIGINS = [(0, 0), (0, 180), (110, 0), (110, 180), (100, 220)]
SEEDS = range(4)
KWARGS = (dict(min_size=0), dict(min_size=30, nms_thresh=0.5), dict(min_size=10, nms_thresh=0.3, max_size=1500))


def tiled_records(seed, n=60):
    g = np.random.default_rng(seed)
    recs = []
    for _ in range(n):
        oy, ox = ORIGINS[g.integers(0, len(ORIGINS))]
        th, tw = min(TILE[0], IMAGE[0] - oy), min(TILE[1], IMAGE[1] - ox)
        m = np.zeros((th, tw), bool)
        cy, cx, r = g.integers(5, th - 5), g.integers(5, tw - 5), g.integers(4, 45)
        yy, xx = np.mgrid[0:th, 0:tw]
        m[(yy - cy) ** 2 + ((xx - cx) * g.uniform(0.6, 1.4)) ** 2 < r * r] = True
        ys, xs = np.nonzero(m)
        bbox = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
        recs.append({"segmentation": m, "bbox": bbox, "global_bbox": [bbox[0] + ox, bbox[1] + oy, bbox[2], bbox[3]],
                     "predicted_iou": float(g.uniform(0.5, 1.0)), "stability_score": float(g.uniform(0.5, 1.0))})
    return recs


def record(mask, origin):
    """A record of ``mask`` (a tile at ``origin`` = (y, x) in the image) the way batched_tiled_inference emits it."""
    ys, xs = np.nonzero(mask)
    bbox = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min()), int(ys.max() - ys.min())]
    return {"segmentation": mask, "bbox": bbox, "global_bbox": [bbox[0] + origin[1], bbox[1] + origin[0], bbox[2], bbox[3]],
            "predicted_iou": 0.9, "stability_score": 0.9}


def pack(mask):
    """bool [th, tw] -> uint32 [ceil(th / 32), tw], bit b of word row yw = row yw * 32 + b, tail bits zero."""
    th, tw = mask.shape
    pad = (-th) % 32
    m = np.pad(mask, ((0, pad), (0, 0))).reshape((th + pad) // 32, 32, tw).astype(np.uint32)
    return (m << np.arange(32, dtype=np.uint32)[None, :, None]).sum(1).astype(np.uint32)


def table(recs):
    """words uint32 [n], word_offset int64 [K], geom int32 [K, 8] = wpc, tw, bx, by, bw, bh, gx, gy."""
    words, offsets, geom, at = [], [], [], 0
    for r in recs:
        w = pack(np.asarray(r["segmentation"]))
        offsets.append(at)
        at += w.size
        words.append(w.ravel())
        geom.append([w.shape[0], w.shape[1]] + [int(v) for v in r["bbox"]] + [int(v) for v in r["global_bbox"][:2]])
    return np.concatenate(words), np.array(offsets, np.int64), np.array(geom, np.int32).reshape(len(recs), 8)


def window(a, b):
    """Intersection window (x0, x1, y0, y1) of the global xywh boxes of two records."""
    ga, gb = a["global_bbox"], b["global_bbox"]
    return (max(ga[0], gb[0]), min(ga[0] + ga[2], gb[0] + gb[2]), max(ga[1], gb[1]), min(ga[1] + ga[3], gb[1] + gb[3]))


def origin(r):
    return r["global_bbox"][1] - r["bbox"][1], r["global_bbox"][0] - r["bbox"][0]            # (y, x) of the record's tile


def overlap(a, b):
    """Pixels set in both masks inside the window, with numpy slices (0 for an empty window)."""
    x0, x1, y0, y1 = window(a, b)
    if x1 <= x0 or y1 <= y0:
        return 0
    (ay, ax), (by, bx) = origin(a), origin(b)
    return int(np.count_nonzero(np.asarray(a["segmentation"])[y0 - ay:y1 - ay, x0 - ax:x1 - ax]
                                & np.asarray(b["segmentation"])[y0 - by:y1 - by, x0 - bx:x1 - bx]))


def candidate_pairs(recs):
    """Every pair i < j whose window is not empty: int32 [Np, 2]."""
    out = []
    for i in range(len(recs)):
        for j in range(i + 1, len(recs)):
            x0, x1, y0, y1 = window(recs[i], recs[j])
            if x1 > x0 and y1 > y0:
                out.append((i, j))
    return np.array(out, np.int32).reshape(-1, 2)


def paint(recs, order, shape):
    """First painter wins, value M - r for record order[r], through the global boxes."""
    label = np.zeros(shape, np.int32)
    for r, k in enumerate(order):
        (bx, by, bw, bh), (gx, gy) = recs[k]["bbox"], recs[k]["global_bbox"][:2]
        m = np.asarray(recs[k]["segmentation"])[by:by + bh, bx:bx + bw]
        view = label[gy:gy + bh, gx:gx + bw]
        view[m & (view == 0)] = len(order) - r
    return label


def same_partition(a, b) -> bool:
    """Two label images split the pixels into the same regions with the same background (a bijection between their values, 0 <-> 0)."""
    if a.shape != b.shape or not np.array_equal(a == 0, b == 0):
        return False
    pairs = np.unique(np.stack([a.ravel(), b.ravel()], axis=1), axis=0)
    return len(set(pairs[:, 0].tolist())) == len(pairs) == len(set(pairs[:, 1].tolist()))


def check_preconditions(recs, oracle):
    """What makes these records a real test of the cross-tile path, asserted on the oracle's / host path's side."""
    shape = oracle.infer_tiled_shape(recs)
    assert shape == (260, 420)
    assert all(r["segmentation"].shape == (150, 200) and pack(r["segmentation"]).shape[0] == 5 for r in recs)
    cross = [(i, j) for i, j in candidate_pairs(recs).tolist()
             if (origin(recs[i])[0] - origin(recs[j])[0]) % 32 != 0 and overlap(recs[i], recs[j]) > 0]
    assert len(cross) >= 48, len(cross)
    tall = sum(r["bbox"][3] > 64 for r in recs)                      # a window of more than 64 rows touches three or more word rows
    assert 9 <= tall <= 14, tall
    for iomin in (False, True):
        lo = oracle.apply_nms([dict(r) for r in recs], min_size=0, nms_thresh=0.5, intersection_over_min=iomin)
        hi = oracle.apply_nms([dict(r) for r in recs], min_size=0, nms_thresh=1.0, intersection_over_min=iomin)
        assert not np.array_equal(lo, hi)
