"""evaluation/multi_dimensional_segmentation.py without a GPU: the default grids, the choice of the seed slices, the dice restatement on
known answers, and the files of the grid search with a stub in place of the model and the propagation."""
import os

import numpy as np
import pandas as pd
import pytest

from micro_sam_amd.evaluation import multi_dimensional_segmentation as MD


def test_default_grid():
    grid = MD.default_grid_search_values_multi_dimensional_segmentation()
    assert list(grid) == ["iou_threshold", "projection", "box_extension"]
    assert grid["iou_threshold"] == [0.5, 0.6, 0.7, 0.8, 0.9]
    assert grid["projection"] == ["mask", "points", "box", "points_and_mask", "single_point"]
    assert grid["box_extension"] == [0.0, 0.025, 0.05, 0.075, 0.1, 0.125, 0.15, 0.175, 0.2, 0.225, 0.25]
    assert len(grid["iou_threshold"]) * len(grid["projection"]) * len(grid["box_extension"]) == 275
    grid = MD.default_grid_search_values_multi_dimensional_segmentation([0.7], ["box"], [0, 3])
    assert grid == {"iou_threshold": [0.7], "projection": ["box"], "box_extension": [0, 3]}


def test_the_package_exports_the_three_functions():
    from micro_sam_amd import evaluation
    for name in ("default_grid_search_values_multi_dimensional_segmentation", "segment_slices_from_ground_truth",
                 "run_multi_dimensional_segmentation_grid_search"):
        assert getattr(evaluation, name) is getattr(MD, name) and name in evaluation.__all__


def _ground_truth():
    gt = np.zeros((7, 20, 24), np.int32)
    gt[0:4, 2:8, 2:8] = 3           # slices 0..3 -> floor(1.5) = 1
    gt[2:7, 10:18, 10:20] = 5       # slices 2..6 -> 4
    gt[6, 0:2, 20:24] = 9           # one slice -> 6, 8 pixels
    gt[1, 15, 2] = 12               # slices 1 and 5 (not contiguous) -> 3, where the object has NO pixel
    gt[5, 15, 2] = 12
    return gt


def test_seed_slices_and_min_size():
    gt = _ground_truth()
    chosen, skipped = MD._select_seed_slices(gt)
    assert chosen == [(3, 1), (5, 4), (9, 6), (12, 3)] and skipped == []
    chosen, skipped = MD._select_seed_slices(gt, min_size=9)
    assert chosen == [(3, 1), (5, 4)] and skipped == [9, 12]
    chosen, skipped = MD._select_seed_slices(gt, min_size=8)
    assert chosen == [(3, 1), (5, 4), (9, 6)] and skipped == [12]
    with pytest.raises(AssertionError):
        MD._select_seed_slices(np.zeros((2, 4, 4), np.int32))


def test_skipped_ids_leave_the_ground_truth_before_scoring():
    gt = _ground_truth()
    assert MD._ground_truth_for_scoring(gt, []) is gt
    cut = MD._ground_truth_for_scoring(gt, [9, 12])
    assert np.unique(cut).tolist() == [0, 3, 5] and np.unique(gt).tolist() == [0, 3, 5, 9, 12]
    assert np.array_equal(cut[gt != 9][gt[gt != 9] != 12], gt[(gt != 9) & (gt != 12)])
    # a segmentation that holds exactly the kept objects is perfect once the skipped ones are gone
    assert MD._score(cut.copy(), gt, [9, 12], "dice") == {"Dice": pytest.approx(1.0, abs=1e-9)}
    assert MD._score(cut.copy(), gt, [], "dice")["Dice"] < 1.0
    with pytest.raises(ValueError, match="not a supported evaluation"):
        MD._score(cut, gt, [], "iou")


def test_dice_on_known_answers():
    a = np.zeros((4, 4), np.int32); b = np.zeros((4, 4), np.int32)
    a[:2] = 7                       # 8 pixels
    b[1:3] = 2                      # 8 pixels, 4 shared
    assert MD.dice_score(a, b) == 2 * 4 / (16 + 1e-7)
    assert MD.dice_score(a, a) == 2 * 8 / (16 + 1e-7)
    assert MD.dice_score(a, np.zeros_like(a)) == 0.0 and MD.dice_score(np.zeros_like(a), np.zeros_like(a)) == 0.0
    assert MD.dice_score(a == 7, b == 2) == 2 * 4 / (16 + 1e-7)               # booleans, as in "dice_per_class"
    assert MD._score(a, b, [], "dice_per_class") == {"Dice": 0.0}             # id 2 is not in the segmentation
    with pytest.raises(ValueError, match="shape"):
        MD.dice_score(a, b[:2])


def test_grid_search_files_with_a_stub_propagator(tmp_path, monkeypatch):
    calls = {"seed": 0, "model": 0, "combos": []}
    gt = _ground_truth()

    def model(*args):
        calls["model"] += 1
        return "predictor", {"features": None}

    def seed(ground_truth, predictor, emb, mode, min_size, verbose):
        calls["seed"] += 1
        assert predictor == "predictor" and mode == "box" and min_size == 8
        return {"skipped": [12]}

    def propagate(seeded, ground_truth, predictor, emb, iou_threshold, projection, box_extension, evaluation_metric="sa", verbose=False):
        calls["combos"].append((iou_threshold, projection, box_extension))
        msa = 0.5 + 0.3 * (projection == "box") - abs(iou_threshold - 0.7) + 0.01 * box_extension
        return {"mSA": msa, "SA50": msa + 0.1, "SA75": msa - 0.1}, np.full(gt.shape, len(calls["combos"]), gt.dtype)

    monkeypatch.setattr(MD, "_model_and_embeddings", model)
    monkeypatch.setattr(MD, "_seed_objects", seed)
    monkeypatch.setattr(MD, "_propagate_and_score", propagate)
    grid = {"iou_threshold": [0.6, 0.7], "projection": ["mask", "box"], "box_extension": [0.0, 0.25]}
    result_dir = str(tmp_path / "gs")
    best = MD.run_multi_dimensional_segmentation_grid_search(np.zeros(gt.shape, np.uint8), gt, "vit_b", None, None, result_dir,
                                                             grid_search_values=grid, min_size=8, store_segmentation=True)
    assert calls["model"] == 1 and calls["seed"] == 1 and len(calls["combos"]) == 8          # loaded and seeded ONCE
    assert calls["combos"][0] == (0.6, "mask", 0.0) and calls["combos"][-1] == (0.7, "box", 0.25)
    assert best == os.path.join(result_dir, "grid_search_params_multi_dimensional_segmentation.csv")
    rows = pd.read_csv(os.path.join(result_dir, "all_grid_search_results.csv"))
    assert len(rows) == 8 and {"mSA", "SA50", "SA75", "iou_threshold", "projection", "box_extension"} <= set(rows.columns)
    top = pd.read_csv(best).iloc[0]
    assert (top["iou_threshold"], top["projection"], top["box_extension"]) == (0.7, "box", 0.25)
    assert top["mSA"] == pytest.approx(0.8025) and top["mSA"] == pytest.approx(rows["mSA"].max())
    assert sorted(os.listdir(os.path.join(result_dir, "predictions"))) == [f"grid_search_result_{i:05}.npy" for i in range(8)]
    assert (np.load(os.path.join(result_dir, "predictions", "grid_search_result_00002.npy")) == 3).all()
    # a second call finds the results and runs nothing
    assert MD.run_multi_dimensional_segmentation_grid_search(None, gt, "vit_b", None, None, result_dir, grid_search_values=grid) == best
    assert calls["model"] == 1 and len(calls["combos"]) == 8
    with pytest.raises(AssertionError, match="three grid-search parameters"):
        MD.run_multi_dimensional_segmentation_grid_search(None, gt, "vit_b", None, None, str(tmp_path / "x"), grid_search_values={"a": [1]})
