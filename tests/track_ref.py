"""The cases and the numpy / scipy references of csrc/track.hip (tests/test_host_track.py, tests/test_gpu_track.py) and of
micro_sam_amd/tracking.py (tests/test_tracking_host.py): ``np.mean`` of ``np.where`` for the centre, ``scipy.ndimage.shift`` for the
shift, and a pure-Python walk of the tracker's control flow driven by a stub "decoder".  TEST INFRASTRUCTURE.

Shapes, chosen for where the kernels can go wrong: (1, 1) one pixel; (31, 7) one partial word row; (32, 64) exactly one word row;
(33, 65) a word row of a single valid row, more columns than a wave; (65, 200) three word rows; (300, 200) H no multiple of 32, ten
word rows.  Up to 70 masks: more than one wave of objects."""
import numpy as np
from scipy import ndimage

import propagate_ref as R

SHAPES = [(1, 1), (31, 7), (32, 64), (33, 65), (65, 200), (300, 200)]
CHUNK = 70                                 # masks per call


def masks(shape, p, seed=0):
    """uint8 [p, H, W] of 0 / 1: empty, full, the single pixel (H - 1, W - 1), then random masks of several densities and blobs."""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w + seed)
    out = np.zeros((p, h, w), np.uint8)
    for i in range(p):
        if i % 8 == 0 and i >= 3:
            yy, xx = np.mgrid[0:h, 0:w]
            cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, h / 2 + 1), rng.uniform(1, w / 2 + 1)
            out[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1.0
        else:
            out[i] = rng.random((h, w)) < (0.5, 0.1, 0.9, 0.02)[i % 4]
    if p >= 1:
        out[0] = 0
    if p >= 2:
        out[1] = 1
    if p >= 3:
        out[2] = 0
        out[2, h - 1, w - 1] = 1
    return out


def moments(m):
    """int64 [P, 3] = (count, sum of y, sum of x) of the pixels that equal 1."""
    out = np.zeros((len(m), 3), np.int64)
    for i, x in enumerate(m):
        ys, xs = np.where(x == 1)
        out[i] = (len(ys), ys.sum(dtype=np.int64), xs.sum(dtype=np.int64))
    return out


def center(mask):
    """The reference's compute_center (micro_sam/sam_annotator/util.py:563-567)."""
    ys, xs = np.where(mask == 1)
    return np.array([np.mean(ys), np.mean(xs)])


def center_from_moments(row):
    """What the tracker forms on the host from one row of the moments."""
    return np.array([np.float64(row[1]) / np.float64(row[0]), np.float64(row[2]) / np.float64(row[0])])


def shift_ref(m, shifts):
    """The reference's _shift_object (:576-579) for every mask."""
    out = np.zeros_like(m)
    for i in range(len(m)):
        ndimage.shift(m[i], tuple(shifts[i]), output=out[i], order=0, prefilter=False)
    return out


def source(n, s):
    """The rule of msam_mask_shift in numpy: source index per output index, -1 where the output is the constant."""
    cc = np.arange(n, dtype=np.float64) - np.float64(s)
    with np.errstate(invalid="ignore"):
        valid = (cc >= 0) & (cc <= n - 1)
        return np.where(valid, np.floor(np.where(valid, cc, 0.0) + 0.5), -1).astype(np.int64)


def offset_varies(n, s):
    """Whether src(i) - i takes more than one value over the valid indices of the axis."""
    src = source(n, s)
    off = (src - np.arange(n))[src >= 0]
    return len(off) > 0 and off.min() != off.max()


def axis_shifts(n):
    """The shifts of one axis of length n: 0, the magnitudes of the list below with both signs, both neighbours of every half-integer
    among them, NaN and the infinities."""
    mags = [0.49, 0.5, 0.51, 1.0, 31.0, 31.5, 32.0, 33.0, float(n - 1), n - 0.5, float(n), 1e6]
    out = [0.0]
    for v in mags:
        out += [v, -v]
    for v in (0.5, 1.5, 31.5, 32.5, n - 0.5):
        for sign in (1.0, -1.0):
            out += [float(np.nextafter(sign * v, np.inf)), float(np.nextafter(sign * v, -np.inf))]
    return out + [float("nan"), float("inf"), float("-inf")]


def shift_pairs(shape, seed=0):
    """float64 [K, 2]: every shift of each axis alone, mixed pairs of the two lists, and random sub-pixel motions."""
    h, w = shape
    ys, xs = axis_shifts(h), axis_shifts(w)
    rng = np.random.default_rng(77 + seed)
    pairs = [(v, 0.0) for v in ys] + [(0.0, v) for v in xs]
    pairs += [(ys[i], xs[(7 * i + 3) % len(xs)]) for i in range(len(ys))]
    pairs += [(rng.uniform(-h, h), rng.uniform(-w, w)) for _ in range(24)]
    pairs += [(rng.uniform(-3, 3), rng.uniform(-3, 3)) for _ in range(16)]
    return np.array(pairs, np.float64)


def shift_batches(shape):
    """[(masks uint8 [p, H, W], shifts float64 [p, 2])]: every pair of ``shift_pairs`` on a mask of ``masks`` (the full and the single
    pixel among them), in calls of at most CHUNK objects."""
    pairs = shift_pairs(shape)
    base = masks(shape, CHUNK, seed=5)
    base[0] = base[3]                                      # (an empty mask shows nothing: a random one in its place)
    out = []
    for s in range(0, len(pairs), CHUNK):
        sh = pairs[s:s + CHUNK]
        out.append((np.ascontiguousarray(base[(np.arange(len(sh)) + s // CHUNK) % CHUNK]), sh))
    return out


def pack(m):
    return R.pack(m)


def unpack(bits, h):
    return R.unpack(bits, h)


def with_garbage_tail(bits, h, seed=3):
    return R.with_garbage_tail(bits, h, seed)


def tail_is_zero(bits, h):
    return h % 32 == 0 or not (bits[:, -1] & ~np.uint32((1 << (h % 32)) - 1)).any()


# ------------------------------------------------------------------------------------------ the tracker's control flow

def stub_decode(shape, t, box, script):
    """The stub "decoder": the rectangle of the box prompt (XYXY, image frame) moved by ``script[t] = (dy, dx, shrink)`` and shrunk by
    ``shrink`` pixels on every side, clipped to the image; ``script[t] = None`` gives an empty mask.  No box: an empty mask."""
    out = np.zeros(shape, bool)
    step = script.get(t, (0, 0, 0))
    if box is None or step is None:
        return out
    dy, dx, shrink = step
    x0, y0, x1, y1 = (int(v) for v in box)
    out[max(y0 + dy + shrink, 0):max(y1 + dy - shrink, 0), max(x0 + dx + shrink, 0):max(x1 + dx - shrink, 0)] = True
    return out


class StubPredictor:
    """Stands in for SamPredictor behind prompt_based_segmentation.segment_from_mask: ``predict`` answers with ``stub_decode`` for the
    frame whose (one-number) embedding util.set_precomputed left in ``features``.  ``calls`` logs (frame, box)."""
    device = "cpu"

    def __init__(self, shape, script):
        self.shape, self.script, self.calls = tuple(shape), script, []
        self.features = None

    def predict(self, point_coords=None, point_labels=None, mask_input=None, box=None, multimask_output=False, return_logits=False):
        t = int(self.features.reshape(-1)[0])
        self.calls.append((t, None if box is None else tuple(int(v) for v in box)))
        return stub_decode(self.shape, t, box, self.script)[None], np.ones(1, np.float32), np.zeros((1, 256, 256), np.float32)


def stub_embeddings(n_frames, shape):
    import torch
    return {"features": torch.arange(n_frames, dtype=torch.float32).reshape(n_frames, 1, 1, 1, 1), "input_size": tuple(shape),
            "original_size": tuple(shape)}


def box_of(mask):
    """_compute_box_from_mask without an extension: XYXY, half-open."""
    ys, xs = np.where(mask == 1)
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1])


def iou(a, b):
    a, b = a == 1, b == 1
    return float((a & b).sum()) / (float((a | b).sum()) + 1e-7)


def walk(seg, frames, stop_upper, threshold, script, alpha=0.5, states=None, log=None):
    """track_from_prompts (reference :582-675) for the box projection, written out step by step on numpy and the stub decoder, with
    the one deviation of micro_sam_amd/tracking.py: the object stops at a frame whose previous mask - or that mask after the shift - is
    empty.  ``log`` collects (frame, what happened, the motion model in use, the box the decoder was prompted with)."""
    seg = seg.copy()
    states = states or {}
    frames = np.asarray(frames)
    log = [] if log is None else log
    has_division = False
    motion = None
    t0 = int(frames.min())
    t = t0 + 1
    while t < seg.shape[0]:
        if not (seg[t - 1] == 1).any():
            log.append((t, "empty", None, None))
            break
        if t == t0 + 2:
            motion = center(seg[t - 1]) - center(seg[t - 2])
        elif t > t0 + 2:
            motion = alpha * motion + (1 - alpha) * (center(seg[t - 1]) - center(seg[t - 2]))
        used = None if motion is None else tuple(motion.tolist())
        box = None
        if t in frames:
            prev, new, state = None, seg[t], states.get(t, "track")
        else:
            prev = seg[t - 1]
            if motion is not None:
                prev = shift_ref(prev[None], motion[None])[0]
            if not (prev == 1).any():
                log.append((t, "shifted out", used, None))
                break
            box = tuple(int(v) for v in box_of(prev))
            new = stub_decode(seg.shape[1:], t, box, script).astype(seg.dtype)
            state = "track"
            if t < frames[-1]:
                prev = None
        if threshold is not None and prev is not None and iou(prev, new) < threshold:
            log.append((t, "gate", used, box))
            break
        if state == "division":
            has_division = True
            log.append((t, "division", used, None))
            break
        seg[t] = new
        log.append((t, "annotated" if t in frames else ("gated" if prev is not None else "tracked"), used, box))
        t += 1
        if t == frames[-1] and stop_upper:
            log.append((t, "stop_upper", None, None))
            break
    return seg, has_division
