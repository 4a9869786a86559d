"""Evaluation of instance segmentations (reference micro_sam/evaluation/evaluation.py): ``run_evaluation`` and
``run_evaluation_for_iterative_prompting`` with the reference's signatures, caching and DataFrame columns, on top of ``matching`` and
``mean_segmentation_accuracy`` - the two functions the reference takes from ``elf.evaluation``, restated here on the device scorer
``ops.label_matching`` (csrc/matching.hip).

The elf semantics, as this module defines them (elf and nifty are not vendored):

* IoU of a (pred object, gt object) pair = c / max(area_p + area_g - c, 1e-7) in float64, from the contingency table.
* ``tp(t)`` = size of a MAXIMUM bipartite matching on the pairs with IoU >= t.  elf solves ``linear_sum_assignment`` on the costs
  ``-(s >= t) - s / (2 n)``; the second term sums to less than 1 over an assignment, so the optimum takes as many pairs above the
  threshold as any matching can, and ``tp`` is that number.  For t > 0.5 the pairs above the threshold already are a matching (two
  objects with IoU > 1/2 against one partner would overlap each other), so ``tp`` is the device's pair count; for t <= 0.5 (the first of
  the default thresholds) it is ``scipy.sparse.csgraph.maximum_bipartite_matching`` on the edge list the device returns.
* fp = n_pred - tp, fn = n_true - tp; precision = tp / (tp + fp), recall = tp / (tp + fn), segmentation_accuracy = tp / (tp + fp + fn),
  f1 = 2 tp / (2 tp + fp + fn), each 0 when tp == 0; mSA = the mean of the accuracies over ``np.arange(0.5, 1., 0.05)``.
* UNPINNED: objects are counted as DISTINCT non-zero ids.  That is elf's count for consecutive ids - what every generator of this
  package and a relabelled ground truth produce; how elf counts sparse ids cannot be checked without it.
* UNPINNED: ground truth read from a FILE is relabelled with ``util._label_equal_value_components`` (4-connected components of equal
  value) where the reference calls ``bioimage_cpp.segmentation.label``; ground truth passed as an array is used as given, as there.
"""
from __future__ import annotations

import os
from glob import glob
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import pandas as pd
import torch
from tqdm import tqdm

from .. import _lib, ops
from ..util import _label_equal_value_components, load_image_data

DEFAULT_THRESHOLDS = np.arange(0.5, 1.0, 0.05)


def _device_labels(labels, device=None) -> torch.Tensor:
    """int32 [1, 1, N] device view / copy of a label image: a numpy array is uploaded, a device tensor is used in place."""
    if isinstance(labels, torch.Tensor):
        if labels.device.type != _lib.require_gpu().type:
            raise ValueError(f"micro_sam_amd: the label tensor lives on {labels.device}; pass a numpy array or a device tensor")
        t = labels if labels.dtype == torch.int32 else labels.to(torch.int32)
    else:
        arr = np.asarray(labels)
        if arr.dtype.kind not in "iub":
            raise TypeError(f"micro_sam_amd: label images must be integers, got {arr.dtype}")
        if arr.dtype != np.int32:
            if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= 2 ** 31):
                raise ValueError("micro_sam_amd: label ids must lie in [0, 2^31)")
            arr = arr.astype(np.int32)
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(_lib.require_gpu(device))
    return t.contiguous().reshape(1, 1, -1)


def _true_positives(counts: np.ndarray, edges: np.ndarray, thresholds: Sequence[float]) -> List[int]:
    tps = []
    for k, t in enumerate(thresholds):
        if t > 0.5 or counts[k] <= 1:
            tps.append(int(counts[k]))                               # the pairs above the threshold are a matching
            continue
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import maximum_bipartite_matching
        score = edges[:, 2] / np.maximum(edges[:, 3] + edges[:, 4] - edges[:, 2], 1e-7)
        e = edges[score >= t]
        assert len(e) == counts[k], "edge list and edge count of the device disagree"
        _, rows = np.unique(e[:, 0], return_inverse=True)
        _, cols = np.unique(e[:, 1], return_inverse=True)
        graph = csr_matrix((np.ones(len(e), np.int8), (rows, cols)), shape=(rows.max() + 1, cols.max() + 1))
        tps.append(int(np.count_nonzero(maximum_bipartite_matching(graph, perm_type="column") >= 0)))
    return tps


def _stats(tp: int, n_pred: int, n_true: int) -> dict:
    fp, fn = n_pred - tp, n_true - tp
    return {"precision": tp / (tp + fp) if tp > 0 else 0, "recall": tp / (tp + fn) if tp > 0 else 0,
            "segmentation_accuracy": tp / (tp + fp + fn) if tp > 0 else 0, "f1": (2 * tp) / (2 * tp + fp + fn) if tp > 0 else 0}


def _score_stack(pred: torch.Tensor, gt: torch.Tensor, thresholds: Sequence[float]) -> List[List[dict]]:
    """Per image of the stack pred [B, ...] (gt [B, ...] or [1, ...]; device int32): the statistics at every threshold, from ONE
    ``ops.label_matching`` call."""
    thresholds = [float(t) for t in thresholds]
    out = []
    for n_pred, n_true, counts, edges in ops.label_matching(pred, gt, thresholds):
        out.append([_stats(tp, n_pred, n_true) for tp in _true_positives(counts, edges, thresholds)])
    return out


def _check_shapes(segmentation, groundtruth):
    if tuple(segmentation.shape) != tuple(groundtruth.shape):
        raise ValueError(f"segmentation and groundtruth differ in shape: {tuple(segmentation.shape)} and {tuple(groundtruth.shape)}")


def matching(segmentation, groundtruth, threshold: float = 0.5) -> dict:
    """``elf.evaluation.matching`` (criterion "iou", background 0 ignored): {"precision", "recall", "segmentation_accuracy", "f1"} of
    the matching at ``threshold``.  Inputs: numpy arrays (uploaded) or device tensors (used in place).  Semantics and what is unpinned
    against the absent library (objects = distinct non-zero ids): the module docstring."""
    _check_shapes(segmentation, groundtruth)
    gt = _device_labels(groundtruth, segmentation.device if isinstance(segmentation, torch.Tensor) else None)
    return _score_stack(_device_labels(segmentation, gt.device), gt, [threshold])[0][0]


def mean_segmentation_accuracy(segmentation, groundtruth, thresholds: Optional[Sequence[float]] = None, return_accuracies: bool = False):
    """``elf.evaluation.mean_segmentation_accuracy``: the mean over ``thresholds`` (default ``np.arange(0.5, 1., 0.05)``) of
    tp / (tp + fp + fn), with the accuracies themselves when ``return_accuracies``.  Inputs and semantics as ``matching``."""
    _check_shapes(segmentation, groundtruth)
    thresholds = DEFAULT_THRESHOLDS if thresholds is None else thresholds
    gt = _device_labels(groundtruth, segmentation.device if isinstance(segmentation, torch.Tensor) else None)
    stats = _score_stack(_device_labels(segmentation, gt.device), gt, thresholds)[0]
    acc = np.array([s["segmentation_accuracy"] for s in stats], dtype=np.float64)
    return (np.mean(acc), acc) if return_accuracies else np.mean(acc)


def _run_evaluation(gt_paths, prediction_paths, verbose=True, thresholds=None):
    assert len(gt_paths) == len(prediction_paths)
    msas, sa50s, sa75s, precisions, recalls, f1s = [], [], [], [], [], []
    for gt_path, pred_path in tqdm(zip(gt_paths, prediction_paths), desc="Evaluate predictions", total=len(gt_paths), disable=not verbose):
        if isinstance(gt_path, np.ndarray):
            gt = gt_path
        else:
            assert os.path.exists(gt_path), gt_path
            gt = _label_equal_value_components(np.asarray(load_image_data(gt_path)))
        if isinstance(pred_path, np.ndarray):
            pred = pred_path
        else:
            assert os.path.exists(pred_path), pred_path
            pred = np.asarray(load_image_data(pred_path))
        assert gt.shape == pred.shape, f"Expected {gt.shape}, got {pred.shape}"
        msa, scores = mean_segmentation_accuracy(pred, gt, thresholds=thresholds, return_accuracies=True)
        stats = matching(pred, gt)
        msas.append(msa)
        if thresholds is None:
            sa50s.append(scores[0])
            sa75s.append(scores[5])
        precisions.append(stats["precision"])
        recalls.append(stats["recall"])
        f1s.append(stats["f1"])
    if thresholds is None:
        return (msas, sa50s, sa75s), (precisions, recalls, f1s)
    return msas, (precisions, recalls, f1s)


def run_evaluation(gt_paths: List[Union[np.ndarray, os.PathLike, str]], prediction_paths: List[Union[np.ndarray, os.PathLike, str]],
                   save_path: Optional[Union[os.PathLike, str]] = None, verbose: bool = True,
                   thresholds: Optional[List[float]] = None) -> pd.DataFrame:
    """Reference ``run_evaluation`` (evaluation/evaluation.py:60-110): one row with mSA, SA50, SA75 (default thresholds only),
    Precision, Recall and "F1 Score", each the mean over the images; an existing ``save_path`` is loaded instead of evaluating."""
    assert len(gt_paths) == len(prediction_paths)
    if save_path is not None and os.path.exists(save_path):
        return pd.read_csv(save_path)
    sas, (precisions, recalls, f1s) = _run_evaluation(gt_paths=gt_paths, prediction_paths=prediction_paths, verbose=verbose, thresholds=thresholds)
    if thresholds is None:
        msas, sa50s, sa75s = sas
    else:
        msas = sas
    results = {"mSA": [np.mean(msas)]}
    if thresholds is None:
        results["SA50"] = [np.mean(sa50s)]
        results["SA75"] = [np.mean(sa75s)]
    results["Precision"] = [np.mean(precisions)]
    results["Recall"] = [np.mean(recalls)]
    results["F1 Score"] = [np.mean(f1s)]
    results = pd.DataFrame.from_dict(results)
    if save_path is not None:
        os.makedirs(Path(save_path).parent, exist_ok=True)
        results.to_csv(save_path, index=False)
    return results


def run_evaluation_for_iterative_prompting(gt_paths: List[Union[os.PathLike, str]], prediction_root: Union[os.PathLike, str],
                                           experiment_folder: Union[os.PathLike, str], start_with_box_prompt: bool = False,
                                           overwrite_results: bool = False, use_masks: bool = False) -> pd.DataFrame:
    """Reference ``run_evaluation_for_iterative_prompting`` (evaluation/evaluation.py:113-167): one row per ``iteration*`` folder of
    ``prediction_root``, written to ``<experiment_folder>/results/iterative_prompting_{with,without}_mask/iterative_prompts_start_
    {box,point}.csv``; returns None when that file exists already (as the reference does)."""
    assert os.path.exists(prediction_root), prediction_root
    result_folder = os.path.join(experiment_folder, "results", "iterative_prompting_" + ("with" if use_masks else "without") + "_mask")
    os.makedirs(result_folder, exist_ok=True)
    csv_path = os.path.join(result_folder, "iterative_prompts_start_box.csv" if start_with_box_prompt else "iterative_prompts_start_point.csv")
    if overwrite_results and os.path.exists(csv_path):
        os.remove(csv_path)
    if os.path.exists(csv_path):
        print(f"Results with iterative prompting for interactive segmentation are already stored at '{csv_path}'.")
        return
    list_of_results = []
    for pred_folder in sorted(glob(os.path.join(prediction_root, "iteration*"))):
        print("Evaluating", os.path.split(pred_folder)[-1])
        pred_paths = sorted(glob(os.path.join(pred_folder, "*")))
        list_of_results.append(run_evaluation(gt_paths=gt_paths, prediction_paths=pred_paths, save_path=None))
    res_df = pd.concat(list_of_results, ignore_index=True)
    res_df.to_csv(csv_path)
    return res_df


def main():
    """@private  The reference's command line (evaluation/evaluation.py:170-256); file lists are ``sorted``, not ``natsorted``."""
    import argparse
    parser = argparse.ArgumentParser(description="Evaluating segmentations from Segment Anything model on custom data.")
    parser.add_argument("--labels", required=True, type=str, nargs="+",
                        help="Filepath(s) to ground-truth labels or the directory where the label data is stored.")
    parser.add_argument("--predictions", required=True, type=str, nargs="+",
                        help="Filepath to predicted labels or the directory where the predicted label data is stored.")
    parser.add_argument("--label_key", type=str, default=None, help="The key for accessing ground-truth label data: a dataset name or a pattern / wildcard.")
    parser.add_argument("--prediction_key", type=str, default=None, help="The key for accessing predicted label data: a dataset name or a pattern / wildcard.")
    parser.add_argument("-o", "--output_path", type=str, default=None, help="The filepath to store the evaluation results (a 'csv' file).")
    parser.add_argument("--threshold", default=None, type=float, nargs="+",
                        help="The overlap threshold(s) for the segmentation accuracy. By default np.arange(0.5, 1., 0.05) is used.")
    parser.add_argument("-v", "--verbose", action="store_true", help="Whether to allow verbosity of evaluation.")
    args = parser.parse_args()

    def _get_inputs_from_paths(paths, key):
        fpaths = []
        for path in paths:
            if os.path.isfile(path):
                fpaths.append(path if key is None else load_image_data(path=path, key=key))
            else:
                assert key is not None, f"You must provide a wildcard / pattern as the filepath '{os.path.abspath(path)}' is a directory."
                fpaths.extend(sorted(glob(os.path.join(path, key))))
        return fpaths

    labels = _get_inputs_from_paths(args.labels, args.label_key)
    predictions = _get_inputs_from_paths(args.predictions, args.prediction_key)
    assert labels and len(labels) == len(predictions)
    output_path = args.output_path
    if output_path is not None:
        if not os.path.isfile(output_path) and not output_path.endswith(".csv"):
            os.makedirs(output_path, exist_ok=True)
            output_path = os.path.join(output_path, "results.csv")
        if not output_path.endswith(".csv"):
            output_path = str(Path(output_path).with_suffix(".csv"))
    results = run_evaluation(gt_paths=labels, prediction_paths=predictions, save_path=output_path, verbose=args.verbose, thresholds=args.threshold)
    print("The evaluation results for the predictions are:")
    print(results)
    if args.verbose and output_path is not None:
        print(f"The evaluation results have been stored at '{os.path.abspath(output_path)}'.")


if __name__ == "__main__":
    main()
