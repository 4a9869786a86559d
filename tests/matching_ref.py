"""Test helper: elf.evaluation.matching / mean_segmentation_accuracy restated with numpy and scipy IN ELF'S OWN FORM - a dense overlap
matrix from ``np.unique`` on the id pairs, intersection over union with elf's ``eps``, and ``linear_sum_assignment`` on elf's cost matrix
``-(s >= t) - s / (2 n)``.  micro_sam_amd.evaluation counts true positives differently (the device's edge counts above 0.5, a maximum
bipartite matching at or below it), so the two formulations check each other.  elf itself is not installed; where its behaviour cannot
be pinned (sparse ids) this file takes the definition the product documents: objects are the DISTINCT non-zero ids.
TEST INFRASTRUCTURE; also the source of the synthetic label images the evaluation tests share."""
import numpy as np
from scipy.optimize import linear_sum_assignment

DEFAULT_THRESHOLDS = np.arange(0.5, 1.0, 0.05)


def contingency(pred, gt):
    """(pred ids, gt ids, dense uint64 overlap matrix [1 + n_pred, 1 + n_true]): row / column 0 is the background whether or not it
    occurs, the others follow the sorted distinct non-zero ids."""
    pred, gt = np.asarray(pred).ravel().astype(np.int64), np.asarray(gt).ravel().astype(np.int64)
    assert pred.shape == gt.shape
    p_ids = np.concatenate([[0], np.setdiff1d(np.unique(pred), [0])])
    g_ids = np.concatenate([[0], np.setdiff1d(np.unique(gt), [0])])
    # the id pairs as one number each (row * columns + column), so that np.unique sorts a flat array
    pairs, counts = np.unique(np.searchsorted(p_ids, pred) * len(g_ids) + np.searchsorted(g_ids, gt), return_counts=True)
    overlap = np.zeros((len(p_ids), len(g_ids)), np.uint64)
    overlap[pairs // len(g_ids), pairs % len(g_ids)] = counts.astype(np.uint64)
    return p_ids, g_ids, overlap


def intersection_over_union(overlap):
    if np.sum(overlap) == 0:
        return overlap.astype(np.float64)
    n_rows = np.sum(overlap, axis=1, keepdims=True)
    n_cols = np.sum(overlap, axis=0, keepdims=True)
    return overlap / np.maximum(n_rows + n_cols - overlap, 1e-7)


def scores(pred, gt):
    """IoU of every (pred object, gt object) pair, background row and column removed: float64 [n_pred, n_true]."""
    return intersection_over_union(contingency(pred, gt)[2])[1:, 1:]


def true_positives(s, threshold):
    n_matched = min(s.shape)
    if n_matched == 0 or not np.any(s >= threshold):
        return 0
    costs = -(s >= threshold).astype(float) - s / (2 * n_matched)
    rows, cols = linear_sum_assignment(costs)
    assert n_matched == len(rows) == len(cols)
    return int(np.count_nonzero(s[rows, cols] >= threshold))


def _stats(tp, n_pred, n_true):
    fp, fn = n_pred - tp, n_true - tp
    return {"precision": tp / (tp + fp) if tp > 0 else 0, "recall": tp / (tp + fn) if tp > 0 else 0,
            "segmentation_accuracy": tp / (tp + fp + fn) if tp > 0 else 0, "f1": (2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0}


def matching(pred, gt, threshold=0.5):
    s = scores(pred, gt)
    return _stats(true_positives(s, threshold), s.shape[0], s.shape[1])


def mean_segmentation_accuracy(pred, gt, thresholds=None, return_accuracies=False):
    s = scores(pred, gt)
    thresholds = DEFAULT_THRESHOLDS if thresholds is None else thresholds
    acc = np.array([_stats(true_positives(s, t), s.shape[0], s.shape[1])["segmentation_accuracy"] for t in thresholds], dtype=np.float64)
    return (np.mean(acc), acc) if return_accuracies else np.mean(acc)


def label_matching(pred, gt, thresholds):
    """What msam_label_matching / ops.label_matching return per batch item, from the dense matrix: [(n_pred, n_true, int64 [T] edge
    counts, int64 [E, 5] edges (pred id, gt id, common pixels, pred area, gt area) with score >= min(t), sorted by (pred id, gt id))]."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    thresholds = np.asarray(thresholds, np.float64)
    out = []
    for b in range(pred.shape[0]):
        p_ids, g_ids, overlap = contingency(pred[b], gt[b if gt.shape[0] > 1 else 0])
        s = intersection_over_union(overlap)[1:, 1:]
        counts = np.array([int(np.count_nonzero((s >= t) & (overlap[1:, 1:] > 0))) for t in thresholds], np.int64)
        area_p, area_g = overlap.sum(1).astype(np.int64), overlap.sum(0).astype(np.int64)
        i, j = np.nonzero((s >= thresholds.min()) & (overlap[1:, 1:] > 0))
        edges = np.stack([p_ids[1:][i], g_ids[1:][j], overlap[1:, 1:][i, j].astype(np.int64), area_p[1:][i], area_g[1:][j]], 1).astype(np.int64) \
            if len(i) else np.zeros((0, 5), np.int64)
        out.append((len(p_ids) - 1, len(g_ids) - 1, counts, edges[np.lexsort((edges[:, 1], edges[:, 0]))]))
    return out


def pair_table(pred, gt):
    """{(pred id, gt id): pixels} with the background pairs: the full contingency table."""
    pred, gt = np.asarray(pred).ravel().astype(np.int64), np.asarray(gt).ravel().astype(np.int64)
    pairs, counts = np.unique(np.stack([pred, gt], 1), axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, counts)}


# ---------------------------------------------------------------------------------------------------------------- label images

def ellipses(H, W, n, seed, shift=(0, 0)):
    """int32 label image of up to ``n`` ellipses (later ones overwrite), drawn ``shift`` pixels away from where seed puts them."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i in range(n):
        cy, cx = rng.uniform(0, H) + shift[0], rng.uniform(0, W) + shift[1]
        ry, rx = rng.uniform(3, H / 6), rng.uniform(3, W / 6)
        lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = i + 1
    return lab


def tie_cases():
    """Exact IoU = 1/2 ties, as (pred, gt, edges at 0.5, tp at 0.5): one prediction of 2k pixels over two gt objects of k; mirrored; a
    chain p1 - g1 - p2 - g2 ... whose maximum matching is smaller than both node counts."""
    k = 12
    pred = np.zeros((4, 16), np.int32)
    gt = np.zeros((4, 16), np.int32)
    pred[1, 2:2 + 2 * k // 2] = 5
    pred[2, 2:2 + 2 * k // 2] = 5                                # 2k pixels in two rows
    gt[1, 2:2 + k] = 3
    gt[2, 2:2 + k] = 4
    one = (pred, gt, 2, 1)
    mirrored = (gt.copy(), pred.copy(), 2, 1)
    # chain: p1 (2k) covers g1, g2 (k each) exactly; p2 and p3 (k each) are exactly covered by g3 (2k):
    # edges at 0.5: p1-g1, p1-g2, p2-g3, p3-g3 -> 3 predictions, 3 gt objects, maximum matching 2
    pc = np.zeros((8, 16), np.int32)
    gc = np.zeros((8, 16), np.int32)
    pc[1:3, 2:2 + k] = 1
    gc[1, 2:2 + k] = 1
    gc[2, 2:2 + k] = 2
    gc[5:7, 2:2 + k] = 3
    pc[5, 2:2 + k] = 2
    pc[6, 2:2 + k] = 3
    return {"one_prediction": one, "mirrored": mirrored, "chain": (pc, gc, 4, 2)}
