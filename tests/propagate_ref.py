"""Host restatement of csrc/propagate.hip for tests/test_host_propagate.py and tests/test_gpu_propagate.py, built on the package's own host
functions (``prompt_based_segmentation._compute_box_from_mask`` / ``_compute_logits_from_mask``, ``util.compute_iou``,
``ResizeLongestSide``), and the case tables both tests share.

Shapes, chosen for where the kernels can go wrong: (300, 200) H no multiple of 32, padded columns, non-dyadic shrink; (96, 160)
enlarging, padded rows; (257, 255) near identity; (256, 256) pass-through; (512, 512) dyadic, exact ties on straight edges;
(768, 1024) scale 4.  P in {1, 3, 14, 70}: seventy is more than one wave of objects."""
import numpy as np
import torch
import torch.nn.functional as F

from micro_sam_amd import util
from micro_sam_amd.prompt_based_segmentation import _compute_box_from_mask, _compute_logits_from_mask
from micro_sam_amd.transforms import ResizeLongestSide

CASES = {"300x200_p70": ((300, 200), 70), "96x160_p14": ((96, 160), 14), "257x255_p1": ((257, 255), 1), "256x256_p3": ((256, 256), 3),
         "512x512_p3": ((512, 512), 3), "768x1024_p3": ((768, 1024), 3)}
BOX_EXTENSIONS = (0, 0.025, 0.25, 3)
TIE_BAND = 1e-5               # |fp64 value - 0.5| below which a pixel of the mask prompt may take either logit
TIE_BAND_MAX_FRACTION = 0.005
HI, LO = np.float32(np.log((1 - 1e-3) / 1e-3)), np.float32(np.log(1e-3 / (1 - 1e-3)))


def _ellipse(shape, rng):
    h, w = shape
    cy, cx = rng.uniform(0.15 * h, 0.85 * h), rng.uniform(0.15 * w, 0.85 * w)
    ry, rx = rng.uniform(0.05 * h, 0.3 * h), rng.uniform(0.05 * w, 0.3 * w)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1.0).astype(np.uint8)


def _specials(shape):
    """empty, full, one pixel in each corner, a one-pixel line in each direction, a square of side 20 (extension 0.025 -> exactly 0.5)."""
    h, w = shape
    out = [np.zeros(shape, np.uint8), np.ones(shape, np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros(shape, np.uint8); m[y, x] = 1; out.append(m)
    m = np.zeros(shape, np.uint8); m[h // 3, :] = 1; out.append(m)
    m = np.zeros(shape, np.uint8); m[:, w // 3] = 1; out.append(m)
    n = min(h, w)
    m = np.zeros(shape, np.uint8); m[np.arange(n), np.arange(n)] = 1; out.append(m)
    m = np.zeros(shape, np.uint8); m[np.arange(n), w - 1 - np.arange(n)] = 1; out.append(m)
    m = np.zeros(shape, np.uint8); m[h - 31:h - 11, 7:27] = 1; out.append(m)
    m = np.zeros(shape, np.uint8); m[5:25, w - 23:w - 3] = 1; out.append(m)
    return out


def masks(name):
    """uint8 [P, H, W]; some pixels hold 2 or 255, which are NOT part of the object (the reference's ``mask == 1``)."""
    shape, p = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    sp = _specials(shape)
    if p >= len(sp):
        out = sp + [_ellipse(shape, rng) for _ in range(p - len(sp))]
    else:
        out = [_ellipse(shape, rng) for _ in range(p)]
        if p > 1:
            out[-1] = sp[rng.integers(2, len(sp))]
    out = np.stack(out)
    other = rng.random(out.shape) < 0.01
    out[other & (out == 0)] = 2
    out[other & (out == 1) & (rng.random(out.shape) < 0.5)] = 255
    if p >= len(sp):
        out[0] = 0; out[1] = 1                       # truly empty / full
        out[10], out[11] = sp[10], sp[11]            # the squares keep their side of 20
    return out


def partners(m, name):
    """A second stack for the IoU: the masks rolled by a few pixels, the empty mask against itself, the full one against itself."""
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    out = np.stack([np.roll(x, (int(rng.integers(-9, 10)), int(rng.integers(-9, 10))), axis=(0, 1)) for x in m])
    if len(m) > 2:
        out[0], out[1] = m[0], m[1]
    return out


def pack(m):
    p, h, w = m.shape
    wpc = (h + 31) // 32
    padded = np.zeros((p, wpc * 32, w), np.uint64)
    padded[:, :h] = m == 1
    sh = np.arange(32, dtype=np.uint64).reshape(1, 1, 32, 1)
    return (padded.reshape(p, wpc, 32, w) << sh).sum(axis=2).astype(np.uint32)


def unpack(bits, h):
    p, wpc, w = bits.shape
    sh = np.arange(32, dtype=np.uint32).reshape(1, 1, 32, 1)
    return (((bits[:, :, None, :] >> sh) & 1).reshape(p, wpc * 32, w)[:, :h]).astype(np.uint8)


def with_garbage_tail(bits, h, seed=3):
    """The same masks with random bits in the rows >= H of the last word row."""
    if h % 32 == 0:
        return bits.copy()
    rng = np.random.default_rng(seed)
    out = bits.copy()
    junk = rng.integers(0, 2 ** 32, size=out[:, -1].shape, dtype=np.uint64).astype(np.uint32)
    out[:, -1] |= junk & ~np.uint32((1 << (h % 32)) - 1)
    return out


def iou(a, b, threshold):
    counts = np.array([[np.logical_and(x == 1, y == 1).sum(), np.logical_or(x == 1, y == 1).sum()] for x, y in zip(a, b)], np.int32)
    keep = np.array([0 if util.compute_iou(x, y) < threshold else 1 for x, y in zip(a, b)], np.uint8)
    return counts, keep


def input_size(shape):
    return ResizeLongestSide.get_preprocess_shape(shape[0], shape[1], 1024)


def boxes(m, box_extension):
    """(nonempty uint8 [P], boxes float32 [P, 4]): the chain of segment_from_mask -> SamPredictor.predict."""
    shape = m.shape[1:]
    nonempty = np.array([(x == 1).any() for x in m], np.uint8)
    out = np.zeros((len(m), 4), np.float32)
    for i, x in enumerate(m):
        if nonempty[i]:
            box = _compute_box_from_mask(x, box_extension=box_extension)
            out[i] = ResizeLongestSide(1024).apply_boxes(box, shape).astype(np.float32)
    return nonempty, out


def resized64(m):
    """float64 [P, 256, 256]: the binary masks resized by torch's CPU operator in fp64 and zero-padded."""
    shape = m.shape[1:]
    th, tw = ResizeLongestSide.get_preprocess_shape(shape[0], shape[1], 256)
    x = torch.from_numpy((m == 1).astype(np.float64))[:, None]
    y = x if (th, tw) == tuple(shape) else F.interpolate(x, (th, tw), mode="bilinear", align_corners=False, antialias=True)
    out = np.zeros((len(m), 256, 256), np.float64)
    out[:, :th, :tw] = y[:, 0].numpy()
    return out


def logits_from(values):
    return np.where(values > 0.5, HI, LO).astype(np.float32)


def tie_band(values):
    return np.abs(values - 0.5) < TIE_BAND


def check_logits(got, values, what=""):
    """Bitwise equal to the thresholded fp64 resize outside the tie band; inside it either logit."""
    band = tie_band(values)
    want = logits_from(values)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isin(got.view(np.uint32), np.array([HI, LO]).view(np.uint32)).all(), what
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~band
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def host_logits(m):
    return np.concatenate([_compute_logits_from_mask(x) for x in m])


def paint(label, m, ids, keep=None):
    out = label.copy()
    for i in np.argsort(ids, kind="stable"):
        if keep is None or keep[i]:
            sel = (m[i] == 1) & (out < ids[i])
            out[sel] = ids[i]
    return out
