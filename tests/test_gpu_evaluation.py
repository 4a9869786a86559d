"""micro_sam_amd.evaluation on the device: ``ops.label_matching`` (csrc/matching.hip) against tests/matching_ref.py (elf's dense overlap
matrix + linear_sum_assignment) on the kernel cases of tests/test_host_label_matching.py - every count and edge equal -, run-to-run
identity, a side stream, the boundary, the two metric functions on numpy and device inputs, and one grid search on the synthetic
vit_b model through both routes (CSV rows equal to each other and to the restatement's scoring of the ``generate()`` outputs)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import matching_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _same(got, want):
    assert len(got) == len(want)
    for b, ((n_pred, n_true, counts, edges), (w_pred, w_true, w_counts, w_edges)) in enumerate(zip(got, want)):
        assert (n_pred, n_true) == (w_pred, w_true), b
        assert np.array_equal(counts, w_counts) and counts.dtype == np.int64, (b, counts, w_counts)
        assert np.array_equal(edges, w_edges) and edges.dtype == np.int64, b


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (pred [B,H,W], gt [G,H,W], thresholds); the references are computed once (``_want``)."""
    ids = np.array([0, 7, 1_000_003, 2 ** 31 - 1], np.int32)
    every = np.arange(1, 4097, dtype=np.int32).reshape(1, 64, 64)
    half = every[:, ::-1].copy() + 5000
    half[0, 32:] = 0
    big_p, big_g = np.zeros((80, 128), np.int32), np.zeros((80, 128), np.int32)
    big_p[5:75, 10:40], big_g[8:78, 12:44], big_p[20:50, 60:120], big_g[25:60, 50:110], big_p[60:, 60:] = 1, 9, 2, 4, 3
    lab = R.ellipses(32, 40, 4, seed=6)
    cases = {
        "ellipses_G1": (np.stack([R.ellipses(96, 128, 20, seed=0, shift=(1 + b, 2 - b)) for b in range(3)]), R.ellipses(96, 128, 20, seed=0)[None], R.DEFAULT_THRESHOLDS),
        "ellipses_GB": (np.stack([R.ellipses(96, 128, 20, seed=b, shift=(1 + b, 2 - b)) for b in range(3)]),
                        np.stack([R.ellipses(96, 128, 20, seed=b) for b in range(3)]), R.DEFAULT_THRESHOLDS),
        "odd_37x53": (R.ellipses(37, 53, 9, seed=3, shift=(1, 1))[None], R.ellipses(37, 53, 9, seed=3)[None], R.DEFAULT_THRESHOLDS),
        "ragged_37x52": (R.ellipses(37, 52, 9, seed=4, shift=(1, 1))[None], R.ellipses(37, 52, 9, seed=4)[None], R.DEFAULT_THRESHOLDS),
        "extreme_ids": (ids[R.ellipses(40, 48, 3, seed=5, shift=(1, 0))][None], ids[[0, 3, 1, 2]][R.ellipses(40, 48, 3, seed=5)][None], [0.3, 0.5]),
        "crowded_lds": (every, half, [0.5, 1.0]),
        "across_workgroups": (big_p[None], big_g[None], [0.3, 0.5, 0.75]),
        "empty_pred": (np.zeros_like(lab)[None], lab[None], R.DEFAULT_THRESHOLDS),
        "empty_gt": (lab[None], np.zeros_like(lab)[None], R.DEFAULT_THRESHOLDS),
        "both_empty": (np.zeros_like(lab)[None], np.zeros_like(lab)[None], R.DEFAULT_THRESHOLDS),
        "sixteen_thresholds": (R.ellipses(48, 64, 12, seed=7, shift=(2, 1))[None], R.ellipses(48, 64, 12, seed=7)[None], np.linspace(0.2, 0.95, 16)),
    }
    for name, (p, g, _, _) in R.tie_cases().items():
        cases["tie_" + name] = (p[None], g[None], [0.5])
    return cases


@functools.lru_cache(maxsize=None)
def _want(name):
    pred, gt, thr = _cases()[name]
    return R.label_matching(pred, gt, thr)


@pytest.mark.parametrize("name", sorted(_cases()))
def test_label_matching_equals_the_restatement(name):
    from micro_sam_amd import ops
    pred, gt, thr = _cases()[name]
    _same(ops.label_matching(_dev(pred), _dev(gt), thr), _want(name))


def test_tables_grow_and_two_runs_are_identical():
    """9216 one-pixel objects against themselves: more pairs than a fresh table has slots and more edges than the first edge list
    holds - the wrapper enlarges both and repeats (the expected result is written down: the dense matrix would be 9216 x 9216); a
    second call on other data returns the same arrays, bit for bit."""
    from micro_sam_amd import _matching, ops
    every = np.arange(1, 9217, dtype=np.int32).reshape(1, 96, 96)
    _matching._MATCH_WS.clear()
    try:
        (n_pred, n_true, counts, edges), = ops.label_matching(_dev(every), _dev(every), [0.5, 1.0])
        state, = _matching._MATCH_WS.values()
        assert state[1] > _matching._MIN_CAPACITY and state[3] >= 9216
    finally:
        _matching._MATCH_WS.clear()
    ids = np.arange(1, 9217, dtype=np.int64)
    assert (n_pred, n_true, list(counts)) == (9216, 9216, [9216, 9216])
    assert np.array_equal(edges, np.stack([ids, ids, np.ones_like(ids), np.ones_like(ids), np.ones_like(ids)], 1))
    pred, gt, thr = _cases()["ellipses_GB"]
    runs = [ops.label_matching(_dev(pred), _dev(gt), thr) for _ in range(2)]
    for x, y in zip(*runs):
        assert x[:2] == y[:2] and x[2].tobytes() == y[2].tobytes() and x[3].tobytes() == y[3].tobytes()


def test_side_stream():
    from micro_sam_amd import ops
    pred, gt, thr = _cases()["ellipses_G1"]
    p, g = _dev(pred), _dev(gt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = ops.label_matching(p, g, thr)
    torch.cuda.current_stream().wait_stream(s)
    _same(got, _want("ellipses_G1"))


def test_boundary():
    from micro_sam_amd import ops
    p = torch.zeros((2, 8, 12), dtype=torch.int32, device="cuda")
    for bad, exc in ((p.long(), TypeError), (p.float(), TypeError), (p.cpu(), ValueError), (torch.zeros((2, 8, 24), dtype=torch.int32, device="cuda")[..., ::2], ValueError),
                     (p[0], ValueError), (p.cpu().numpy(), TypeError)):
        with pytest.raises(exc, match="pred"):
            ops.label_matching(bad, p, [0.5])
        if isinstance(bad, torch.Tensor) and bad.dim() == 3:
            with pytest.raises(exc, match="gt"):
                ops.label_matching(p, bad, [0.5])
    with pytest.raises(ValueError, match="gt"):
        ops.label_matching(p, torch.zeros((3, 8, 12), dtype=torch.int32, device="cuda"), [0.5])
    with pytest.raises(ValueError, match="thresholds"):
        ops.label_matching(p, p, [0.5] * 17)


def test_metrics_numpy_and_device_inputs_equal_the_restatement():
    from micro_sam_amd.evaluation import evaluation as E
    pairs = [(R.ellipses(96, 128, 20, seed=0, shift=(2, 1)), R.ellipses(96, 128, 20, seed=0))]
    pairs += [(p, g) for p, g, _, _ in R.tie_cases().values()]
    lab = R.ellipses(32, 40, 4, seed=6)
    pairs += [(np.zeros_like(lab), lab), (lab, lab)]
    for pred, gt in pairs:
        w_msa, w_acc = R.mean_segmentation_accuracy(pred, gt, return_accuracies=True)
        for a, b in ((pred, gt), (_dev(pred), _dev(gt)), (pred.astype(np.uint32), gt.astype(np.int64)), (_dev(pred), gt)):
            msa, acc = E.mean_segmentation_accuracy(a, b, return_accuracies=True)
            assert msa == w_msa and np.array_equal(acc, w_acc)
            for t in (0.3, 0.5, 0.75):
                assert E.matching(a, b, t) == R.matching(pred, gt, t)
    assert E.mean_segmentation_accuracy(pairs[0][0], pairs[0][1], thresholds=[0.25, 0.5]) == R.mean_segmentation_accuracy(pairs[0][0], pairs[0][1], [0.25, 0.5])


def test_grid_search_fast_and_general_routes_write_the_same_rows(tmp_path, vit_b_sd):
    """One 1024 x 1024 synthetic tile, points_per_side=8, a 2 x 2 grid: the fast path (generate_device per combination, one
    label_matching call for the stack) and the reference's route (generate() forced through its general path, scored per image)
    write equal CSVs, and both equal the restatement's scoring of the generate() outputs."""
    from micro_sam_amd import ops, util
    from micro_sam_amd.evaluation import instance_segmentation as I
    from micro_sam_amd.instance_segmentation import AutomaticMaskGenerator
    from micro_sam_amd.synthetic import synthetic_tile_with_labels
    image, gt = synthetic_tile_with_labels(3)
    predictor = util.get_sam_model("vit_b", device="cuda:0", state_dict=vit_b_sd)
    amg = AutomaticMaskGenerator(predictor, points_per_side=8)
    grid = {"pred_iou_thresh": [0.0, 0.7], "stability_score_thresh": [0.0, 0.8]}
    calls = []
    real = ops.label_matching
    ops.label_matching = lambda p, g, t: (calls.append(tuple(p.shape)), real(p, g, t))[1]
    try:
        I.run_instance_segmentation_grid_search(amg, grid, [image], [gt], str(tmp_path / "fast"), None)
        assert [c[0] for c in calls] == [4], calls                      # the fast path: ONE call for the four combinations
        amg._general_generate = True
        I.run_instance_segmentation_grid_search(amg, grid, [image], [gt], str(tmp_path / "general"), None,
                                                fixed_generate_kwargs={"min_mask_region_area": 0})
        assert [c[0] for c in calls[1:]] == [1] * 8
    finally:
        ops.label_matching = real
    fast = pd.read_csv(tmp_path / "fast" / "image_0.csv", float_precision="round_trip")
    general = pd.read_csv(tmp_path / "general" / "image_0.csv", float_precision="round_trip")
    assert (tmp_path / "fast" / "image_0.csv").read_text() == (tmp_path / "general" / "image_0.csv").read_text()
    assert list(fast.columns) == ["image_name", "mSA", "SA50", "SA75", "Precision", "Recall", "F1", "pred_iou_thresh", "stability_score_thresh"]
    amg.initialize(image)
    rows = iter(fast.itertuples())
    n_objects = []
    for iou in grid["pred_iou_thresh"]:
        for stab in grid["stability_score_thresh"]:
            seg = amg.generate(pred_iou_thresh=iou, stability_score_thresh=stab, min_mask_region_area=0)
            n_objects.append(int(seg.max()))
            msa, acc = R.mean_segmentation_accuracy(seg, gt, return_accuracies=True)
            st = R.matching(seg, gt)
            row = next(rows)
            assert (row.mSA, row.SA50, row.SA75, row.Precision, row.Recall, row.F1, row.pred_iou_thresh, row.stability_score_thresh) == \
                (msa, acc[0], acc[5], st["precision"], st["recall"], st["f1"], iou, stab)
    assert general.equals(fast) and max(n_objects) >= 2
