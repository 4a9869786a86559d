"""Grid search and inference for the automatic instance segmentation (reference micro_sam/evaluation/instance_segmentation.py): the
reference's signatures, CSV columns (``image_name, mSA, SA50, SA75, Precision, Recall, F1``, then the parameters), file names and
skip-if-exists behaviour.

Differences that follow from this environment: images and ground truth may be given as paths (read with ``util.load_image_data``) or
as arrays (named ``image_{i}``), and predictions are written as ``<stem>.npy`` (imageio is not vendored).

The grid search has two routes that write identical rows.  The reference's: ``generate()`` per combination, scored on its own.  The
fast one, for an ``AutomaticMaskGenerator`` with a single-crop device state and parameters ``generate_device`` takes: the label images
of a chunk of combinations stay on the device, are stacked and scored against the ONE uploaded ground truth with a single
``ops.label_matching`` call per chunk (csrc/matching.hip), and the convergence flags of the chunk are read once."""
from __future__ import annotations

import inspect
import os
from glob import glob
from itertools import product
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import pandas as pd
import torch
from tqdm import tqdm

from .. import util
from ..instance_segmentation import AMGBase, AutomaticMaskGenerator, InstanceSegmentationWithDecoder
from . import evaluation as _ev

_STACK_BYTES = 256 << 20            # label images of one scoring chunk


def _get_range_of_search_values(input_vals, step):
    """``[first, last]`` -> the values from first to last INCLUSIVE in steps of ``step``, rounded to 3 digits; a scalar -> [scalar].
    The reference writes ``np.arange(first, last + step, step)``, whose length depends on how ``last + step`` rounds: for [0.6, 0.9]
    and 0.025 it yields a 14th value, 0.925, outside the range its docstring gives.  Here the number of steps is counted first, so
    the defaults are the documented 13 x 15 grid."""
    if isinstance(input_vals, list):
        n = int(round((input_vals[1] - input_vals[0]) / step)) + 1
        search_range = [round(float(input_vals[0] + i * step), 3) for i in range(n)]
    else:
        search_range = [input_vals]
    return search_range


def default_grid_search_values_amg(iou_thresh_values: Optional[List[float]] = None,
                                   stability_score_values: Optional[List[float]] = None) -> Dict[str, List[float]]:
    """Default grid for AMG: ``pred_iou_thresh`` from 0.6 to 0.9 and ``stability_score_thresh`` from 0.6 to 0.95, steps of 0.025
    (13 x 15 combinations)."""
    if iou_thresh_values is None:
        iou_thresh_values = _get_range_of_search_values([0.6, 0.9], step=0.025)
    if stability_score_values is None:
        stability_score_values = _get_range_of_search_values([0.6, 0.95], step=0.025)
    return {"pred_iou_thresh": iou_thresh_values, "stability_score_thresh": stability_score_values}


def default_grid_search_values_instance_segmentation_with_decoder(
    center_distance_threshold_values: Optional[List[float]] = None, boundary_distance_threshold_values: Optional[List[float]] = None,
    distance_smoothing_values: Optional[List[float]] = None, min_size_values: Optional[List[float]] = None,
) -> Dict[str, List[float]]:
    """Default grid for the decoder-based instance segmentation: both distance thresholds from 0.3 to 0.7 in steps of 0.1,
    ``distance_smoothing`` from 1.0 to 2.0 in steps of 0.2, ``min_size`` 50, 100 and 200."""
    if center_distance_threshold_values is None:
        center_distance_threshold_values = _get_range_of_search_values([0.3, 0.7], step=0.1)
    if boundary_distance_threshold_values is None:
        boundary_distance_threshold_values = _get_range_of_search_values([0.3, 0.7], step=0.1)
    if distance_smoothing_values is None:
        distance_smoothing_values = _get_range_of_search_values([1.0, 2.0], step=0.2)
    if min_size_values is None:
        min_size_values = [50, 100, 200]
    return {"center_distance_threshold": center_distance_threshold_values, "boundary_distance_threshold": boundary_distance_threshold_values,
            "distance_smoothing": distance_smoothing_values, "min_size": min_size_values}


def default_grid_search_values_apg(
    min_distance_values: Optional[List[float]] = None, threshold_abs_values: Optional[List[float]] = None,
    multimasking_values: Optional[List[float]] = None, prompt_selection_values: Optional[List[float]] = None,
    min_size_values: Optional[List[float]] = None, nms_threshold_values: Optional[List[float]] = None,
    intersection_over_min_values: Optional[List[bool]] = None, mask_threshold_values: Optional[List[Union[float, str]]] = None,
    center_distance_threshold_values: Optional[List[float]] = None, boundary_distance_threshold_values: Optional[List[float]] = None,
) -> Dict[str, List[float]]:
    """Default grid for APG; as in the reference only the connected-component parameters, ``min_size``, ``nms_threshold`` and
    ``intersection_over_min`` are searched (the other arguments are accepted and unused there too)."""
    if center_distance_threshold_values is None:
        center_distance_threshold_values = _get_range_of_search_values([0.3, 0.7], step=0.1)
    if boundary_distance_threshold_values is None:
        boundary_distance_threshold_values = _get_range_of_search_values([0.3, 0.7], step=0.1)
    if min_size_values is None:
        min_size_values = [50, 100, 200]
    if nms_threshold_values is None:
        nms_threshold_values = _get_range_of_search_values([0.5, 0.9], step=0.1)
    if intersection_over_min_values is None:
        intersection_over_min_values = [True, False]
    return {"center_distance_threshold": center_distance_threshold_values, "boundary_distance_threshold": boundary_distance_threshold_values,
            "min_size": min_size_values, "nms_threshold": nms_threshold_values, "intersection_over_min": intersection_over_min_values}


def _row(image_name: str, stats: List[dict], gs_kwargs: Dict[str, Any]) -> Dict[str, Any]:
    """One CSV row from the statistics at the default thresholds (index 0 = 0.5, index 5 = 0.75)."""
    acc = np.array([s["segmentation_accuracy"] for s in stats], dtype=np.float64)
    row = {"image_name": image_name, "mSA": np.mean(acc), "SA50": acc[0], "SA75": acc[5], "Precision": stats[0]["precision"],
           "Recall": stats[0]["recall"], "F1": stats[0]["f1"]}
    row.update(gs_kwargs)
    return row


def _general_row(segmenter, gs_kwargs, fixed_generate_kwargs, gt, image_name):
    instance_labels = segmenter.generate(**(gs_kwargs | fixed_generate_kwargs))
    m_sas, sas = _ev.mean_segmentation_accuracy(instance_labels, gt, return_accuracies=True)
    stats = _ev.matching(instance_labels, gt)
    row = {"image_name": image_name, "mSA": m_sas, "SA50": sas[0], "SA75": sas[5], "Precision": stats["precision"],
           "Recall": stats["recall"], "F1": stats["f1"]}
    row.update(gs_kwargs)
    return row


# what generate() and generate_device() both take
_DEVICE_PARAMS = tuple(p for p in inspect.signature(AutomaticMaskGenerator.generate_device).parameters
                       if p != "self" and p in inspect.signature(AutomaticMaskGenerator.generate).parameters)


def _fast_path(segmenter, gs_combinations, fixed_generate_kwargs) -> bool:
    """An AutomaticMaskGenerator with a single-crop device state whose parameters are all ``generate_device``'s
    (``min_mask_region_area=0`` is its behaviour; any other value is not)."""
    if not isinstance(segmenter, AutomaticMaskGenerator) or getattr(segmenter, "_general_generate", False):
        return False
    crops = getattr(segmenter, "_crop_list", None)
    if not segmenter.is_initialized or crops is None or len(crops) != 1 or "bits" not in crops[0] or len(crops[0]) == 0:
        return False
    for kw in list(gs_combinations) + [fixed_generate_kwargs]:
        for k, v in kw.items():
            if k == "min_mask_region_area":
                if v != 0:
                    return False
            elif k == "output_mode":
                if v != "instance_segmentation":
                    return False
            elif k not in _DEVICE_PARAMS:
                return False
    return True


def _grid_search_iteration(segmenter: Union[AMGBase, InstanceSegmentationWithDecoder], gs_combinations: List[Dict], gt: np.ndarray,
                           image_name: str, fixed_generate_kwargs: Dict[str, Any], result_path: Optional[Union[str, os.PathLike]],
                           verbose: bool = False) -> pd.DataFrame:
    rows: List[Optional[Dict[str, Any]]] = [None] * len(gs_combinations)
    if _fast_path(segmenter, gs_combinations, fixed_generate_kwargs):
        gt_dev = _ev._device_labels(gt, segmenter._predictor.device)                 # uploaded once, [1, 1, N]
        n_px = int(gt_dev.numel())
        if tuple(gt.shape) != tuple(segmenter.original_size):
            raise ValueError(f"ground truth {tuple(gt.shape)} and image {tuple(segmenter.original_size)} differ in shape")
        chunk = max(1, min(_STACK_BYTES // (4 * n_px), 1024))
        drop = ("min_mask_region_area", "output_mode")
        for start in tqdm(range(0, len(gs_combinations), chunk), disable=not verbose):
            combos = gs_combinations[start:start + chunk]
            stack = torch.empty((len(combos), 1, n_px), dtype=torch.int32, device=gt_dev.device)
            flags = []
            for j, gs_kwargs in enumerate(combos):
                kw = {k: v for k, v in (gs_kwargs | fixed_generate_kwargs).items() if k not in drop}
                labels, flag = segmenter.generate_device(**kw)
                stack[j, 0].copy_(labels.reshape(-1))
                flags.append(flag)
            stats = _ev._score_stack(stack, gt_dev, _ev.DEFAULT_THRESHOLDS)          # one library call, one download
            flags = torch.cat(flags).cpu().numpy()                                    # the convergence flags, once per chunk
            for j, gs_kwargs in enumerate(combos):
                rows[start + j] = _row(image_name, stats[j], gs_kwargs) if flags[j] == 0 else \
                    _general_row(segmenter, gs_kwargs, fixed_generate_kwargs, gt, image_name)
    else:
        for j, gs_kwargs in enumerate(tqdm(gs_combinations, disable=not verbose)):
            rows[j] = _general_row(segmenter, gs_kwargs, fixed_generate_kwargs, gt, image_name)
    img_gs_df = pd.concat([pd.DataFrame([r]) for r in rows])
    img_gs_df.to_csv(result_path, index=False)
    return img_gs_df


def _load_image(path, key, roi):
    im = util.load_image_data(path, key=key)
    return np.asarray(im) if roi is None else np.asarray(im[roi])


def _named(item, i: int) -> Tuple[str, bool]:
    """(name, is an array) of an image / ground-truth entry: the file's stem, or ``image_{i}`` for an array."""
    if isinstance(item, np.ndarray):
        return f"image_{i}", True
    return Path(item).stem, False


def run_instance_segmentation_grid_search(
    segmenter: Union[AMGBase, InstanceSegmentationWithDecoder], grid_search_values: Dict[str, List],
    image_paths: List[Union[str, os.PathLike, np.ndarray]], gt_paths: List[Union[str, os.PathLike, np.ndarray]],
    result_dir: Union[str, os.PathLike], embedding_dir: Optional[Union[str, os.PathLike]],
    fixed_generate_kwargs: Optional[Dict[str, Any]] = None, verbose_gs: bool = False, image_key: Optional[str] = None,
    gt_key: Optional[str] = None, rois: Optional[Tuple[slice, ...]] = None,
    tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None,
) -> None:
    """Reference ``run_instance_segmentation_grid_search`` (evaluation/instance_segmentation.py:218-321): every combination of
    ``grid_search_values`` (parameters of the segmenter's ``generate``) is run on every image after ONE ``initialize`` and scored
    against the ground truth; one ``<image name>.csv`` per image in ``result_dir``, images whose file exists are skipped.  Images and
    ground truth: paths or arrays (``image_{i}``).  See the module docstring for the two routes."""
    verbose_embeddings = False
    assert len(image_paths) == len(gt_paths)
    fixed_generate_kwargs = {} if fixed_generate_kwargs is None else fixed_generate_kwargs
    duplicate_params = [gs_param for gs_param in grid_search_values.keys() if gs_param in fixed_generate_kwargs]
    if duplicate_params:
        raise ValueError("You may not pass duplicate parameters in 'grid_search_values' and 'fixed_generate_kwargs'."
                         f"The parameters {duplicate_params} are duplicated.")
    gs_combinations = [{k: v for k, v in zip(grid_search_values.keys(), vals)} for vals in product(*grid_search_values.values())]
    os.makedirs(result_dir, exist_ok=True)
    predictor = getattr(segmenter, "_predictor", None)
    for i, (image_path, gt_path) in tqdm(enumerate(zip(image_paths, gt_paths)), desc="Run instance segmentation grid-search", total=len(image_paths)):
        image_name, image_is_array = _named(image_path, i)
        result_path = os.path.join(result_dir, f"{image_name}.csv")
        if os.path.exists(result_path):
            continue
        roi = None if rois is None else rois[i]
        if image_is_array:
            image = image_path if roi is None else image_path[roi]
        else:
            assert os.path.exists(image_path), image_path
            image = _load_image(image_path, image_key, roi=roi)
        if isinstance(gt_path, np.ndarray):
            gt = gt_path if roi is None else gt_path[roi]
        else:
            assert os.path.exists(gt_path), gt_path
            gt = _load_image(gt_path, gt_key, roi=roi)
        if tiling_window_params is None:
            tiling_window_params = {}
        if embedding_dir is None:
            segmenter.initialize(image, **tiling_window_params)
        else:
            assert predictor is not None
            embedding_path = os.path.join(embedding_dir, f"{os.path.splitext(image_name)[0]}.zarr")
            image_embeddings = util.precompute_image_embeddings(predictor, image, embedding_path, ndim=2, verbose=verbose_embeddings,
                                                                **tiling_window_params)
            segmenter.initialize(image, image_embeddings, **tiling_window_params)
        _grid_search_iteration(segmenter, gs_combinations, gt, image_name, fixed_generate_kwargs=fixed_generate_kwargs,
                               result_path=result_path, verbose=verbose_gs)


def run_instance_segmentation_inference(
    segmenter: Union[AMGBase, InstanceSegmentationWithDecoder], image_paths: List[Union[str, os.PathLike, np.ndarray]],
    embedding_dir: Optional[Union[str, os.PathLike]], prediction_dir: Union[str, os.PathLike],
    generate_kwargs: Optional[Dict[str, Any]] = None, tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None,
) -> None:
    """Reference ``run_instance_segmentation_inference`` (:324-377): ``initialize`` + ``generate(**generate_kwargs)`` per image, the
    label image written to ``<prediction_dir>/<stem>.npy`` (the reference writes a compressed image file of the input's name through
    imageio); images whose prediction exists are skipped."""
    verbose_embeddings = False
    generate_kwargs = {} if generate_kwargs is None else generate_kwargs
    predictor = segmenter._predictor
    os.makedirs(prediction_dir, exist_ok=True)
    for i, image_path in enumerate(tqdm(image_paths, desc="Run inference for automatic mask generation")):
        image_name, image_is_array = _named(image_path, i)
        prediction_path = os.path.join(prediction_dir, f"{image_name}.npy")
        if os.path.exists(prediction_path):
            continue
        if image_is_array:
            image = image_path
        else:
            assert os.path.exists(image_path), image_path
            image = _load_image(image_path, None, roi=None)
        if embedding_dir is None:
            embedding_path = None
        else:
            assert predictor is not None
            embedding_path = os.path.join(embedding_dir, f"{image_name}.zarr")
        if tiling_window_params is None:
            tiling_window_params = {}
        image_embeddings = util.precompute_image_embeddings(predictor, image, embedding_path, ndim=2, verbose=verbose_embeddings,
                                                            **tiling_window_params)
        segmenter.initialize(image, image_embeddings, **tiling_window_params)
        instances = segmenter.generate(**generate_kwargs)
        np.save(prediction_path, np.asarray(instances))


def evaluate_instance_segmentation_grid_search(result_dir: Union[str, os.PathLike], grid_search_parameters: List[str],
                                               criterion: str = "mSA") -> Tuple[Dict[str, Any], float]:
    """Reference ``evaluate_instance_segmentation_grid_search`` (:380-410): the parameter setting with the best mean ``criterion``
    over the per-image CSVs of ``result_dir``, and that score."""
    gs_files = glob(os.path.join(result_dir, "*.csv"))
    gs_result = pd.concat([pd.read_csv(gs_file) for gs_file in gs_files])
    gs_result = gs_result[grid_search_parameters + [criterion]].reset_index()
    grouped_result = gs_result.groupby(grid_search_parameters).mean().reset_index()
    best_score, best_idx = grouped_result[criterion].max(), grouped_result[criterion].idxmax()
    best_params = grouped_result.iloc[best_idx]
    assert np.isclose(best_params[criterion], best_score)
    best_kwargs = {k: v for k, v in zip(grid_search_parameters, best_params)}
    return best_kwargs, best_score


def save_grid_search_best_params(best_kwargs, best_msa, grid_search_result_dir=None):
    """Reference ``save_grid_search_best_params`` (:413-428), file names included."""
    param_df = pd.DataFrame.from_dict([best_kwargs])
    res_df = pd.DataFrame.from_dict([{"best_msa": best_msa}])
    best_param_df = pd.merge(res_df, param_df, left_index=True, right_index=True)
    path_name = "grid_search_params_amg.csv" if "pred_iou_thresh" and "stability_score_thresh" in best_kwargs \
        else "grid_search_params_instance_segmentation_with_decoder.csv"
    if grid_search_result_dir is not None:
        os.makedirs(os.path.join(grid_search_result_dir, "results"), exist_ok=True)
        res_path = os.path.join(grid_search_result_dir, "results", path_name)
    else:
        res_path = path_name
    best_param_df.to_csv(res_path)


def run_instance_segmentation_grid_search_and_inference(
    segmenter: Union[AMGBase, InstanceSegmentationWithDecoder], grid_search_values: Dict[str, List],
    val_image_paths: List[Union[str, os.PathLike]], val_gt_paths: List[Union[str, os.PathLike]],
    test_image_paths: List[Union[str, os.PathLike]], embedding_dir: Optional[Union[str, os.PathLike]],
    prediction_dir: Union[str, os.PathLike], experiment_folder: Union[str, os.PathLike], result_dir: Union[str, os.PathLike],
    fixed_generate_kwargs: Optional[Dict[str, Any]] = None, verbose_gs: bool = True,
    tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None,
) -> None:
    """Reference ``run_instance_segmentation_grid_search_and_inference`` (:431-498): grid search on the validation images, the best
    setting saved under ``<experiment_folder>/results``, inference with it on the test images."""
    run_instance_segmentation_grid_search(
        segmenter=segmenter, grid_search_values=grid_search_values, image_paths=val_image_paths, gt_paths=val_gt_paths,
        result_dir=result_dir, embedding_dir=embedding_dir, fixed_generate_kwargs=fixed_generate_kwargs, verbose_gs=verbose_gs,
        tiling_window_params=tiling_window_params)
    best_kwargs, best_msa = evaluate_instance_segmentation_grid_search(result_dir, list(grid_search_values.keys()))
    best_param_str = ", ".join(f"{k} = {v}" for k, v in best_kwargs.items())
    print("Best grid-search result:", best_msa, "with parmeters:\n", best_param_str)
    print()
    save_grid_search_best_params(best_kwargs, best_msa, experiment_folder)
    generate_kwargs = {} if fixed_generate_kwargs is None else fixed_generate_kwargs
    generate_kwargs.update(best_kwargs)
    if "prompt_selection" in generate_kwargs:
        generate_kwargs["prompt_selection"] = _maybe_list_value(generate_kwargs["prompt_selection"])
    run_instance_segmentation_inference(
        segmenter=segmenter, image_paths=test_image_paths, embedding_dir=embedding_dir, prediction_dir=prediction_dir,
        generate_kwargs=generate_kwargs, tiling_window_params=tiling_window_params)


def _maybe_list_value(val):
    if not isinstance(val, str):
        return val
    s = val.strip()
    if s.startswith("[") and s.endswith("]"):
        import ast
        parsed = ast.literal_eval(s)
        if isinstance(parsed, list):
            return parsed
    return val
