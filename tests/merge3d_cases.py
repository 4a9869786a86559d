"""Test helper of tests/test_merge3d_host.py and tests/test_gpu_merge3d.py: the label volumes the gap closing of csrc/merge3d.hip is
checked on, and the yardstick - the host functions of micro_sam_amd.multi_dimensional_segmentation on the same arrays.  TEST
INFRASTRUCTURE.  Every case is (name, labels int32 [Z, H, W], gap)."""
import numpy as np


def _disc(img, cy, cx, r, value):
    yy, xx = np.ogrid[: img.shape[0], : img.shape[1]]
    img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def _running(slices):
    """Per-slice label images with ids 1..k -> a volume with the running offsets of segment_slices."""
    out, offset = [], 0
    for s in slices:
        s = s.astype(np.int32)
        out.append(np.where(s > 0, s + offset, 0))
        offset += int(s.max())
    return np.stack(out).astype(np.int32)


def case_blobs():
    """1: blobs that wander a little from slice to slice, a blank middle slice; the sides are no multiples of the tile."""
    rng = np.random.default_rng(3)
    centres = [(int(rng.integers(8, 88)), int(rng.integers(8, 72)), int(rng.integers(3, 9))) for _ in range(14)]
    slices = []
    for z in range(5):
        img = np.zeros((96, 80), np.int32)
        if z != 2:
            for k, (cy, cx, r) in enumerate(centres):
                if (k + z) % 5 == 0:
                    continue                       # an object that misses a slice
                _disc(img, cy + (z % 2), cx + z // 2, r, k + 1)
            ids = np.unique(img[img > 0])
            img = np.searchsorted(ids, img).astype(np.int32) + (img > 0)
        slices.append(img)
    return _running(slices)


def _wide_layout(shift=0):
    img = np.zeros((40, 600), np.int32)
    img[2:9, 530 + shift:561 + shift] = 1          # first raster pixel beyond column 512
    img[5:13, 100 + shift:131 + shift] = 2         # starts later, inside the first 512 columns
    y = 26
    for x in range(5, 596):                        # a snake of diagonal steps across every tile column and two tile rows
        img[y, x] = 3
        if x % 2 == 0:
            y += 1 if (x // 24) % 2 == 0 else -1
    img[30:38, 300:340] = 4
    return img


def case_wide():
    """2: linear against block-major order beyond 512 columns, a component across many tile borders."""
    slices = []
    for z in range(7):
        img = _wide_layout(z % 2)
        if z == 3:
            img[img == 3] = 0                      # the snake misses a slice: a bridged gap (gap 1) / stays open (not for gap 2)
            img[img == 1] = 0
        if z == 2:
            img[img == 4] = 0
        slices.append(img)
    return _running([np.where(s > 0, np.searchsorted(np.unique(s[s > 0]), s) + 1, 0) for s in slices])


def case_painting_order():
    """3: slice 2 holds two objects with a one-pixel gap under one large object of slices 1 and 3 (one closed component, two labels),
    an object in two pieces - one inside that component, one alone (a kept component that is painted over completely) - and two
    ordinary objects before and after it in raster order."""
    vol = np.zeros((5, 48, 48), np.int32)
    for z, base in ((0, 0), (1, 10), (3, 30), (4, 40)):
        vol[z, 10:31, 5:41] = base + 1
        vol[z, 40:45, 30:37] = base + 2
    s = vol[2]
    s[1:5, 1:5] = 21
    s[12:29, 8:21] = 22
    s[12:29, 22:35] = 23
    s[14:19, 36:40] = 24                           # piece inside the merging component
    s[40:45, 5:11] = 24                            # piece alone
    s[40:45, 30:37] = 25
    return vol


def case_diagonal():
    """4: two squares of different labels that touch at one corner only: one 8-connected component with two labels."""
    vol = np.zeros((3, 12, 14), np.int32)
    vol[1, 2:5, 2:5] = 3
    vol[1, 5:8, 5:8] = 4
    vol[1, 8:10, 3:5] = 5                          # touches label 4's square at a corner as well (the other diagonal)
    vol[0, 2:5, 9:12] = 1
    vol[2, 2:5, 9:12] = 6
    return vol


def case_bridged():
    """5: an object of slices 0 and 2 leaves a component without any label in slice 1."""
    vol = np.zeros((4, 16, 18), np.int32)
    vol[0, 3:9, 3:9] = 1
    vol[2, 4:10, 2:8] = 3
    vol[1, 11:15, 10:16] = 2
    vol[3, 3:9, 3:9] = 4
    return vol


def case_all_edge():
    """6: 2 gap >= Z: every slice is only renumbered."""
    rng = np.random.default_rng(6)
    vol = np.zeros((4, 33, 65), np.int32)
    for z in range(4):
        for k in range(6):
            _disc(vol[z], int(rng.integers(3, 30)), int(rng.integers(3, 62)), int(rng.integers(2, 5)), 10 * z + 2 * k + 3)
    return vol


def case_empty_slices():
    """7: an empty first slice and an empty interior slice (no bridge either)."""
    vol = np.zeros((5, 20, 24), np.int32)
    vol[1, 2:8, 2:8] = 1
    vol[3, 12:18, 14:20] = 2
    vol[4, 12:18, 14:20] = 3
    vol[4, 2:6, 2:6] = 4
    return vol


def case_reset():
    """7b: gap 2 - the empty slice 1 is an edge slice: the offset falls back to 1 and the ids of slice 0 come again."""
    vol = np.zeros((6, 20, 24), np.int32)
    vol[0, 2:8, 2:8] = 1
    vol[0, 12:18, 14:20] = 2
    for z in (2, 3, 4, 5):
        vol[z, 3:9, 3:9] = 2 * z + 1
        vol[z, 12:18, 12:20] = 2 * z + 2
    return vol


def case_repeating_ids():
    """8: ids that are not consecutive and come again in every slice."""
    vol = np.zeros((4, 24, 30), np.int32)
    for z in range(4):
        vol[z, 2:8, 2 + z:9 + z] = 17
        vol[z, 10:16, 12:20] = 5
        if z != 2:
            vol[z, 17:22, 3:27] = 40
    return vol


def case_single_slice():
    """9: Z = 1."""
    vol = np.zeros((1, 10, 70), np.int32)
    vol[0, 1:4, 1:6] = 9
    vol[0, 5:9, 60:69] = 2
    return vol


def cases():
    wide = case_wide()
    return [("blobs", case_blobs(), 1), ("wide_gap1", wide, 1), ("wide_gap2", wide, 2), ("painting_order", case_painting_order(), 1),
            ("diagonal", case_diagonal(), 1), ("bridged", case_bridged(), 1), ("all_edge", case_all_edge(), 2),
            ("empty_slices", case_empty_slices(), 1), ("reset", case_reset(), 2), ("repeating_ids", case_repeating_ids(), 1),
            ("single_slice", case_single_slice(), 1)]


CASE_NAMES = ["blobs", "wide_gap1", "wide_gap2", "painting_order", "diagonal", "bridged", "all_edge", "empty_slices", "reset",
              "repeating_ids", "single_slice"]


def host_close(labels: np.ndarray, gap: int):
    """(volume, final offset) of the host's _preprocess_closing.  The final offset is restated from the function's own loop: it is what
    the next slice would have started at."""
    from micro_sam_amd.multi_dimensional_segmentation import _preprocess_closing
    out = _preprocess_closing(labels, gap)
    Z = labels.shape[0]
    offset = 1
    for z in range(Z):
        m = int(out[z].max())
        if z < gap or z >= Z - gap:
            offset = m + 1
        elif m > 0:
            offset = m + 1
    return out, offset


def z_ranges_ref(labels: np.ndarray, n_ids: int) -> np.ndarray:
    Z = labels.shape[0]
    zr = np.empty((n_ids, 2), np.int32)
    zr[:, 0], zr[:, 1] = Z, -1
    for z in range(Z):
        ids = np.unique(labels[z])
        ids = ids[(ids > 0) & (ids < n_ids)]
        zr[ids, 0] = np.minimum(zr[ids, 0], z)
        zr[ids, 1] = np.maximum(zr[ids, 1], z)
    return zr
