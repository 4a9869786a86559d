"""micro_sam_amd.evaluation without a device: ``ops.label_matching`` is replaced by a numpy stand-in built on the restatement's
contingency table (tests/matching_ref.label_matching), so what runs is the host side - true positives from edge counts / maximum
matching against elf's linear_sum_assignment form, the metric formulas, the DataFrame columns, CSV caching and skip-if-exists, the
choice of the best grid point, the grid defaults - plus the boundary of the real ``ops.label_matching`` under the recorder of
tests/ops_boundary_table.py (a refusal is a ValueError / TypeError that names the argument, before any library call)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import matching_ref as R
from ops_boundary_table import recording


@pytest.fixture()
def ev(monkeypatch):
    from micro_sam_amd import _lib, ops
    from micro_sam_amd.evaluation import evaluation
    calls = []

    def stand_in(pred, gt, thresholds):
        calls.append((tuple(pred.shape), tuple(gt.shape), len(thresholds)))
        assert pred.dtype == torch.int32 and gt.dtype == torch.int32 and pred.dim() == 3
        return R.label_matching(pred.numpy(), gt.numpy(), thresholds)
    monkeypatch.setattr(ops, "label_matching", stand_in)
    monkeypatch.setattr(_lib, "require_gpu", lambda device=None: torch.device("cpu"))
    evaluation.calls = calls
    return evaluation


def _pairs():
    out = [(R.ellipses(48, 64, 12, seed=s, shift=(2, 1)), R.ellipses(48, 64, 12, seed=s)) for s in range(3)]
    out += [(p, g) for p, g, _, _ in R.tie_cases().values()]
    lab = R.ellipses(32, 40, 4, seed=6)
    out += [(np.zeros_like(lab), lab), (lab, np.zeros_like(lab)), (np.zeros_like(lab), np.zeros_like(lab)), (lab, lab)]
    return out


def test_metrics_equal_the_restatement(ev):
    for pred, gt in _pairs():
        for t in (0.3, 0.5, 0.75):
            assert ev.matching(pred, gt, t) == R.matching(pred, gt, t)
        msa, acc = ev.mean_segmentation_accuracy(pred, gt, return_accuracies=True)
        w_msa, w_acc = R.mean_segmentation_accuracy(pred, gt, return_accuracies=True)
        assert msa == w_msa and np.array_equal(acc, w_acc) and acc.dtype == np.float64 and len(acc) == 10
        assert ev.mean_segmentation_accuracy(pred, gt, thresholds=[0.2, 0.5, 0.9]) == R.mean_segmentation_accuracy(pred, gt, [0.2, 0.5, 0.9])
        assert ev.mean_segmentation_accuracy(torch.from_numpy(pred), torch.from_numpy(gt)) == w_msa            # tensors are used in place
    assert set(ev.matching(*_pairs()[0])) == {"precision", "recall", "segmentation_accuracy", "f1"}


def test_formulas_and_tp_zero(ev):
    s = ev._stats(3, 5, 4)
    assert s == {"precision": 3 / 5, "recall": 3 / 4, "segmentation_accuracy": 3 / 6, "f1": 6 / 9}
    assert ev._stats(0, 5, 4) == {"precision": 0, "recall": 0, "segmentation_accuracy": 0, "f1": 0}
    assert ev._stats(0, 0, 0)["f1"] == 0
    pred, gt, edges, tp = R.tie_cases()["chain"]
    st = ev.matching(pred, gt, 0.5)                                     # 4 edges at 0.5, maximum matching 2 of 3 and 3 objects
    assert st["precision"] == 2 / 3 and st["recall"] == 2 / 3 and st["segmentation_accuracy"] == 2 / 4
    with pytest.raises(ValueError):
        ev.matching(np.zeros((3, 4), np.int32), np.zeros((4, 3), np.int32))
    with pytest.raises(ValueError):
        ev.matching(np.full((3, 4), -1, np.int64), np.zeros((3, 4), np.int64))
    with pytest.raises(TypeError):
        ev.matching(np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32))


def test_run_evaluation_columns_and_caching(ev, tmp_path):
    pairs = _pairs()[:3]
    gts, preds = [g for _, g in pairs], [p for p, _ in pairs]
    for i, p in enumerate(preds):
        np.save(tmp_path / f"pred_{i}.npy", p)
    save = tmp_path / "out" / "results.csv"
    df = ev.run_evaluation(gts, [str(tmp_path / f"pred_{i}.npy") for i in range(3)], save_path=str(save), verbose=False)
    assert list(df.columns) == ["mSA", "SA50", "SA75", "Precision", "Recall", "F1 Score"] and len(df) == 1
    want = [R.mean_segmentation_accuracy(p, g, return_accuracies=True) for p, g in pairs]
    assert df["mSA"][0] == np.mean([w[0] for w in want]) and df["SA50"][0] == np.mean([w[1][0] for w in want])
    assert df["SA75"][0] == np.mean([w[1][5] for w in want])
    assert df["F1 Score"][0] == np.mean([R.matching(p, g)["f1"] for p, g in pairs])
    n = len(ev.calls)
    again = ev.run_evaluation(gts, preds, save_path=str(save), verbose=False)                   # the file exists: loaded, nothing scored
    assert len(ev.calls) == n and np.allclose(again.values, df.values)
    df2 = ev.run_evaluation(gts, preds, verbose=False, thresholds=[0.5, 0.6])
    assert list(df2.columns) == ["mSA", "Precision", "Recall", "F1 Score"]
    # a ground truth read from a file is relabelled into connected components of equal value
    split = np.zeros((8, 8), np.int32)
    split[1:3, 1:3] = 1
    split[5:7, 5:7] = 1
    np.save(tmp_path / "gt.npy", split)
    two = split.copy()
    two[5:7, 5:7] = 2
    assert ev.run_evaluation([str(tmp_path / "gt.npy")], [two], verbose=False)["mSA"][0] == 1.0
    assert ev.run_evaluation([split], [two], verbose=False)["mSA"][0] < 1.0                        # an array is used as given


def test_iterative_prompting_evaluation(ev, tmp_path):
    pred, gt = _pairs()[0]
    for it in range(2):
        os.makedirs(tmp_path / "pred" / f"iteration{it:02}")
        np.save(tmp_path / "pred" / f"iteration{it:02}" / "a.npy", pred if it else gt)
    df = ev.run_evaluation_for_iterative_prompting([gt], str(tmp_path / "pred"), str(tmp_path / "exp"), start_with_box_prompt=True)
    csv = tmp_path / "exp" / "results" / "iterative_prompting_without_mask" / "iterative_prompts_start_box.csv"
    assert csv.exists() and len(df) == 2 and df["mSA"][0] == 1.0 and df["mSA"][1] == R.mean_segmentation_accuracy(pred, gt)
    assert ev.run_evaluation_for_iterative_prompting([gt], str(tmp_path / "pred"), str(tmp_path / "exp"), start_with_box_prompt=True) is None


class _Segmenter:
    """generate() = the stored label image with the objects whose id exceeds ``keep`` removed."""
    _predictor = None

    def __init__(self):
        self.initialized = 0

    def initialize(self, image, **kw):
        self.initialized += 1
        self.image = image

    def generate(self, keep=100, offset=0):
        out = self.image.copy()
        out[out > keep] = 0
        return out


def test_grid_search_general_route_csv_and_skip(ev, tmp_path):
    from micro_sam_amd.evaluation import instance_segmentation as I
    gt = R.ellipses(48, 64, 12, seed=1)
    image = R.ellipses(48, 64, 12, seed=1, shift=(1, 1))
    np.save(tmp_path / "img0.npy", image)
    seg = _Segmenter()
    grid = {"keep": [3, 6, 100]}
    I.run_instance_segmentation_grid_search(seg, grid, [str(tmp_path / "img0.npy"), image], [gt, gt], str(tmp_path / "res"), None,
                                            fixed_generate_kwargs={"offset": 0})
    assert sorted(os.listdir(tmp_path / "res")) == ["image_1.csv", "img0.csv"] and seg.initialized == 2
    df = pd.read_csv(tmp_path / "res" / "img0.csv", float_precision="round_trip")      # (the default parser is an ulp off)
    assert list(df.columns) == ["image_name", "mSA", "SA50", "SA75", "Precision", "Recall", "F1", "keep"] and len(df) == 3
    for k, row in zip(grid["keep"], df.itertuples()):
        pred = seg.generate(keep=k)
        msa, acc = R.mean_segmentation_accuracy(pred, gt, return_accuracies=True)
        st = R.matching(pred, gt)
        assert (row.mSA, row.SA50, row.SA75, row.Precision, row.Recall, row.F1, row.keep) == (msa, acc[0], acc[5], st["precision"], st["recall"], st["f1"], k)
    I.run_instance_segmentation_grid_search(seg, grid, [str(tmp_path / "img0.npy")], [gt], str(tmp_path / "res"), None)
    assert seg.initialized == 2                                                              # the CSV exists: skipped
    with pytest.raises(ValueError, match="duplicate"):
        I.run_instance_segmentation_grid_search(seg, grid, [image], [gt], str(tmp_path / "res2"), None, fixed_generate_kwargs={"keep": 1})
    best, score = I.evaluate_instance_segmentation_grid_search(str(tmp_path / "res"), ["keep"])
    assert best == {"keep": 100} and np.isclose(score, df["mSA"].max())


def test_evaluate_grid_search_on_hand_written_csvs(tmp_path):
    from micro_sam_amd.evaluation import instance_segmentation as I
    cols = "image_name,mSA,SA50,SA75,Precision,Recall,F1,pred_iou_thresh,stability_score_thresh\n"
    (tmp_path / "a.csv").write_text(cols + "a,0.5,0.6,0.4,1,1,1,0.6,0.7\na,0.7,0.8,0.5,1,1,1,0.8,0.7\na,0.1,0.8,0.5,1,1,1,0.8,0.9\n")
    (tmp_path / "b.csv").write_text(cols + "b,0.9,0.6,0.4,1,1,1,0.6,0.7\nb,0.5,0.8,0.5,1,1,1,0.8,0.7\nb,0.2,0.9,0.5,1,1,1,0.8,0.9\n")
    best, score = I.evaluate_instance_segmentation_grid_search(str(tmp_path), ["pred_iou_thresh", "stability_score_thresh"])
    assert best == {"pred_iou_thresh": 0.6, "stability_score_thresh": 0.7} and np.isclose(score, 0.7)
    best, score = I.evaluate_instance_segmentation_grid_search(str(tmp_path), ["pred_iou_thresh", "stability_score_thresh"], criterion="SA50")
    assert best == {"pred_iou_thresh": 0.8, "stability_score_thresh": 0.9} and np.isclose(score, 0.85)
    I.save_grid_search_best_params(best, score, str(tmp_path / "exp"))
    saved = pd.read_csv(tmp_path / "exp" / "results" / "grid_search_params_amg.csv")
    assert saved["best_msa"][0] == score and saved["pred_iou_thresh"][0] == 0.8


def test_grid_defaults():
    from micro_sam_amd.evaluation import instance_segmentation as I
    a, b = I._get_range_of_search_values([0.6, 0.9], 0.025), I._get_range_of_search_values([0.6, 0.95], 0.025)
    assert len(a) == 13 and len(b) == 15 and a[0] == 0.6 and a[-1] == 0.9 and b[-1] == 0.95 and a[1] == 0.625
    assert I._get_range_of_search_values(0.7, 0.1) == [0.7]
    amg = I.default_grid_search_values_amg()
    assert list(amg) == ["pred_iou_thresh", "stability_score_thresh"] and [len(v) for v in amg.values()] == [13, 15]
    dec = I.default_grid_search_values_instance_segmentation_with_decoder()
    assert {k: len(v) for k, v in dec.items()} == {"center_distance_threshold": 5, "boundary_distance_threshold": 5, "distance_smoothing": 6, "min_size": 3}
    apg = I.default_grid_search_values_apg()
    assert list(apg) == ["center_distance_threshold", "boundary_distance_threshold", "min_size", "nms_threshold", "intersection_over_min"]
    assert I.default_grid_search_values_amg(iou_thresh_values=[0.5])["pred_iou_thresh"] == [0.5]


def test_inference_writes_npy_and_skips(ev, tmp_path, monkeypatch):
    from micro_sam_amd import util
    from micro_sam_amd.evaluation import instance_segmentation as I
    monkeypatch.setattr(util, "precompute_image_embeddings", lambda predictor, image, path, **kw: None)
    seg = _Segmenter()
    seg.initialize = lambda image, emb=None, **kw: (_Segmenter.initialize(seg, image))
    image = R.ellipses(24, 24, 5, seed=2)
    np.save(tmp_path / "cells.npy", image)
    I.run_instance_segmentation_inference(seg, [str(tmp_path / "cells.npy"), image], None, str(tmp_path / "pred"), {"keep": 2})
    assert sorted(os.listdir(tmp_path / "pred")) == ["cells.npy", "image_1.npy"]
    assert np.array_equal(np.load(tmp_path / "pred" / "cells.npy"), seg.generate(keep=2))
    n = seg.initialized
    I.run_instance_segmentation_inference(seg, [str(tmp_path / "cells.npy")], None, str(tmp_path / "pred"))
    assert seg.initialized == n


# ------------------------------------------------------------------------------------------------- the boundary of ops.label_matching

def test_label_matching_boundary_under_the_recorder():
    from micro_sam_amd import ops
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt)                      # noqa: E731
    faults = {
        "pred": [z(2, 4, 6, dt=torch.int64), z(2, 4, 12)[..., ::2], z(1, 2, 4, 6), z(2, 4, 6).to("meta"), np.zeros((2, 4, 6), np.int32)],
        "gt": [z(2, 4, 6, dt=torch.float32), z(2, 4, 12)[..., ::2], z(3, 4, 6), z(2, 4, 5), z(2, 4, 6).to("meta"), None],
        "thresholds": [[], [0.5] * 17, [float("nan")]],
    }
    for name, values in faults.items():
        for v in values:
            kw = dict(pred=z(2, 4, 6), gt=z(2, 4, 6), thresholds=[0.5, 0.75])
            kw[name] = v
            with recording() as rec:
                with pytest.raises((ValueError, TypeError), match=name):
                    ops.label_matching(**kw)
            assert not rec.calls, (name, rec.names())
    with recording() as rec:                                                     # valid arguments reach the one entry point
        rec.ZERO = dict(rec.ZERO, msam_label_matching=lambda a: (a[11], 4 * (4 + 2 * 20)))
        out = ops.label_matching(z(2, 4, 6), z(1, 4, 6), [0.5, 0.75])
    assert rec.names() == ["msam_label_matching"] and len(out) == 2 and out[0][:2] == (0, 0) and out[0][3].shape == (0, 5)
    a = rec.calls[0][1]
    assert a[2:6] == [2, 1, 4, 6] and a[7] == 2 and a[10] >= 1024 and a[10] & (a[10] - 1) == 0 and a[9] >= 64
