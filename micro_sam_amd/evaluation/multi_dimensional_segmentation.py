"""Evaluation and grid search of the interactive 3-d segmentation (reference micro_sam/evaluation/multi_dimensional_segmentation.py):
every object of a labelled volume is seeded in its middle slice from the ground truth, carried through the volume, and the result
is scored.  Names, parameters, defaults, result keys and file names are the reference's; what differs:

* all objects are carried at once by ``multi_dimensional_segmentation.segment_objects_in_volume`` (one batched decode per slice on
  the device for box / mask projections) instead of one ``segment_mask_in_volume`` call per object, and the objects seeded in one
  slice share one batched decode;
* the grid search loads the model, the embeddings and the seeds ONCE - none depends on the grid - where the reference reloads the
  model for every combination;
* two trailing keywords ``predictor`` / ``image_embeddings`` let a caller supply the model;
* volumes are saved as ``.npy`` (imageio is absent, as in ``evaluation/instance_segmentation.py``);
* scoring runs on the device (``evaluation.mean_segmentation_accuracy`` takes the label volume as one image); ``elf``'s
  ``dice_score`` is restated (``dice_score`` below; UNPINNED against the absent library).
"""
from __future__ import annotations

import os
from itertools import product
from math import floor
from typing import Dict, List, Literal, Optional, Tuple, Union

import numpy as np
import pandas as pd
import torch
from tqdm import tqdm

from .. import util
from .instance_segmentation import _get_range_of_search_values, evaluate_instance_segmentation_grid_search


def default_grid_search_values_multi_dimensional_segmentation(
    iou_threshold_values: Optional[List[float]] = None, projection_method_values: Optional[Union[str, dict]] = None,
    box_extension_values: Optional[Union[float, int]] = None,
) -> Dict[str, List]:
    """Reference :22-55: ``iou_threshold`` from 0.5 to 0.9 in steps of 0.1, the five projections, ``box_extension`` from 0 to 0.25 in
    steps of 0.025 (5 x 5 x 11 combinations)."""
    if iou_threshold_values is None:
        iou_threshold_values = _get_range_of_search_values([0.5, 0.9], step=0.1)
    if projection_method_values is None:
        projection_method_values = ["mask", "points", "box", "points_and_mask", "single_point"]
    if box_extension_values is None:
        box_extension_values = _get_range_of_search_values([0, 0.25], step=0.025)
    return {"iou_threshold": iou_threshold_values, "projection": projection_method_values, "box_extension": box_extension_values}


def dice_score(segmentation, groundtruth, threshold_seg: Optional[float] = 0, threshold_gt: Optional[float] = 0,
               eps: float = 1e-7) -> float:
    """``elf.evaluation.dice_score`` restated: 2 |A n B| / (|A| + |B| + eps) with A = segmentation > threshold_seg and
    B = groundtruth > threshold_gt (a threshold of None takes the input as it is)."""
    seg = np.asarray(segmentation.cpu() if torch.is_tensor(segmentation) else segmentation)
    gt = np.asarray(groundtruth.cpu() if torch.is_tensor(groundtruth) else groundtruth)
    if seg.shape != gt.shape:
        raise ValueError(f"segmentation and groundtruth differ in shape: {seg.shape} and {gt.shape}")
    a = seg > threshold_seg if threshold_seg is not None else seg
    b = gt > threshold_gt if threshold_gt is not None else gt
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(2.0 * (a * b).sum() / (a.sum() + b.sum() + eps))


def _select_seed_slices(ground_truth: np.ndarray, min_size: int = 0) -> Tuple[List[Tuple[int, int]], List[int]]:
    """Reference :113-138: per object id (ascending, without the first - the background) the middle slice
    floor(mean(z_min, z_max)) of its extent; objects with fewer than ``min_size`` pixels in that slice are skipped.
    Returns ([(label_id, slice)], [skipped ids])."""
    label_ids = np.unique(ground_truth)[1:]
    assert len(label_ids) > 0, "There are no objects to perform volumetric segmentation."
    chosen, skipped = [], []
    for label_id in label_ids:
        zs = np.flatnonzero((ground_truth == label_id).any(axis=(1, 2)))
        slice_choice = floor(np.mean((zs.min(), zs.max())))
        if min_size > 0 and int((ground_truth[slice_choice] == label_id).sum()) < min_size:
            skipped.append(int(label_id))
            continue
        chosen.append((int(label_id), int(slice_choice)))
    return chosen, skipped


def _ground_truth_for_scoring(ground_truth: np.ndarray, skipped_label_ids) -> np.ndarray:
    """Reference :207-211: the skipped objects do not count as misses."""
    if not len(skipped_label_ids):
        return ground_truth
    curr_gt = ground_truth.copy()
    curr_gt[np.isin(curr_gt, skipped_label_ids)] = 0
    return curr_gt


def _seed_objects(ground_truth, predictor, image_embeddings, interactive_seg_mode: str = "box", min_size: int = 0,
                  verbose: bool = False):
    """The prompt-based segmentation of every object in its middle slice (reference :124-181): a box, or one positive and one negative
    point, from ``PointAndBoxPromptGenerator`` on the ground truth; the objects of one slice are decoded in one batch, and each
    object's seed is what ``batched_inference`` returns for its prompt alone (the first connected component of its mask).
    The connected components of a seed are numbered through ``inference._records_to_segmentation_device``, which hands a host array
    back: one small round trip per object, once per volume (not per grid combination).
    Returns dict(seeds uint8 [N, H, W] on the device, seed_slices [N], ids [N], skipped [..])."""
    from ..inference import _records_to_segmentation_device, batched_inference
    from ..prompt_generators import PointAndBoxPromptGenerator
    from .. import ops
    if interactive_seg_mode == "points":
        get_points, get_box = True, False
    elif interactive_seg_mode == "box":
        get_points, get_box = False, True
    else:
        raise ValueError(f"The provided interactive prompting '{interactive_seg_mode}' for the first slice isn't supported. "
                         "Please choose from 'box' / 'points'.")
    chosen, skipped = _select_seed_slices(ground_truth, min_size)
    generator = PointAndBoxPromptGenerator(n_positive_points=1 if get_points else 0, n_negative_points=1 if get_points else 0,
                                           dilation_strength=10, get_point_prompts=get_points, get_box_prompts=get_box)
    shape = tuple(ground_truth.shape[1:])
    seeds = torch.zeros((len(chosen),) + shape, dtype=torch.uint8, device=predictor.device)
    by_slice: Dict[int, List[int]] = {}
    for n, (_, z) in enumerate(chosen):
        by_slice.setdefault(z, []).append(n)
    for z, members in tqdm(sorted(by_slice.items()), desc="Segmenting the objects in their middle slices", disable=not verbose):
        boxes, points, point_labels = [], [], []
        for n in members:
            this_slice_seg = (ground_truth[z] == chosen[n][0]).astype("int")
            _, box_coords = util.get_centers_and_bounding_boxes(this_slice_seg)
            p, l, b, _ = generator(segmentation=torch.from_numpy(this_slice_seg)[None, None].to(torch.float32),
                                   bbox_coordinates=[box_coords[1]])
            if get_box:
                boxes.append(np.asarray(b).reshape(4))
            else:
                points.append(np.asarray(p).reshape(-1, 2))
                point_labels.append(np.asarray(l).reshape(-1))
        util.set_precomputed(predictor, image_embeddings, i=z)
        records = batched_inference(predictor, None, batch_size=max(1, len(members)), boxes=np.stack(boxes) if get_box else None,
                                    points=np.stack(points) if get_points else None,
                                    point_labels=np.stack(point_labels) if get_points else None, return_instance_segmentation=False)
        for n, rec in zip(members, records):
            bits = ops.pack_bits(rec["segmentation"][None].contiguous())
            single = _records_to_segmentation_device(bits, rec["area"].reshape(1), shape)       # batched_inference of this prompt alone
            seeds[n] = torch.from_numpy((single == 1).astype(np.uint8)).to(seeds.device)
    return {"seeds": seeds, "seed_slices": np.array([z for _, z in chosen], dtype=np.int64),
            "ids": np.array([i for i, _ in chosen], dtype=np.int64), "skipped": skipped}


def _score(final_segmentation, ground_truth: np.ndarray, skipped, evaluation_metric: str) -> Dict[str, float]:
    """Reference :206-237.  ``final_segmentation``: a label volume, numpy or on the device."""
    from .evaluation import mean_segmentation_accuracy
    curr_gt = _ground_truth_for_scoring(ground_truth, skipped)
    if evaluation_metric == "sa":
        msa, sa = mean_segmentation_accuracy(final_segmentation, curr_gt, return_accuracies=True)
        return {"mSA": msa, "SA50": sa[0], "SA75": sa[5]}
    seg = final_segmentation.cpu().numpy() if torch.is_tensor(final_segmentation) else final_segmentation
    if evaluation_metric == "dice":
        return {"Dice": dice_score(seg, curr_gt)}
    if evaluation_metric == "dice_per_class":
        return {"Dice": float(np.mean([dice_score(seg == i, curr_gt == i) for i in np.unique(curr_gt)[1:]]))}
    raise ValueError(f"'{evaluation_metric}' is not a supported evaluation metrics. Please choose 'sa' / 'dice' / 'dice_per_class'.")


def _propagate_and_score(seeded, ground_truth, predictor, image_embeddings, iou_threshold, projection, box_extension,
                         evaluation_metric: str = "sa", verbose: bool = False):
    from ..multi_dimensional_segmentation import segment_objects_in_volume
    labels, _ = segment_objects_in_volume(predictor, image_embeddings, seeded["seeds"], seeded["seed_slices"], seeded["ids"],
                                          iou_threshold=iou_threshold, projection=projection, box_extension=box_extension,
                                          return_device=True, verbose=verbose)
    results = _score(labels, ground_truth, seeded["skipped"], evaluation_metric)
    return results, labels.cpu().numpy().astype(ground_truth.dtype)


def _model_and_embeddings(volume, model_type, checkpoint_path, embedding_path, device, verbose, predictor, image_embeddings):
    if predictor is None:
        predictor = util.get_sam_model(model_type=model_type, checkpoint_path=checkpoint_path, device=device)
    if image_embeddings is None:
        image_embeddings = util.precompute_image_embeddings(predictor=predictor, input_=volume, save_path=embedding_path, ndim=3,
                                                            verbose=verbose)
    return predictor, image_embeddings


@torch.no_grad()
def segment_slices_from_ground_truth(
    volume: np.ndarray, ground_truth: np.ndarray, model_type: str, checkpoint_path: Optional[Union[str, os.PathLike]] = None,
    embedding_path: Optional[Union[str, os.PathLike]] = None, save_path: Optional[Union[str, os.PathLike]] = None,
    iou_threshold: float = 0.8, projection: Union[str, dict] = "mask", box_extension: Union[float, int] = 0.025,
    device: Union[str, torch.device] = None, interactive_seg_mode: str = "box", verbose: bool = False,
    return_segmentation: bool = False, min_size: int = 0, evaluation_metric: Literal["sa", "dice"] = "sa",
    predictor=None, image_embeddings=None,
) -> Union[Dict, Tuple[Dict, np.ndarray]]:
    """Reference ``segment_slices_from_ground_truth`` (:58-242): every object of ``ground_truth`` is segmented from a box (or points)
    in its middle slice, carried through the volume, and the label volume is scored: {"mSA", "SA50", "SA75"} for "sa", {"Dice"} for
    "dice" / "dice_per_class".  An existing ``save_path`` (``.npy``) is loaded instead of segmenting."""
    assert volume.ndim == 3
    if save_path is not None and os.path.exists(save_path):
        _, skipped = _select_seed_slices(ground_truth, min_size)
        final_segmentation = np.load(save_path)
        results = _score(final_segmentation, ground_truth, skipped, evaluation_metric)
    else:
        predictor, image_embeddings = _model_and_embeddings(volume, model_type, checkpoint_path, embedding_path, device, verbose,
                                                            predictor, image_embeddings)
        seeded = _seed_objects(ground_truth, predictor, image_embeddings, interactive_seg_mode, min_size, verbose)
        results, final_segmentation = _propagate_and_score(seeded, ground_truth, predictor, image_embeddings, iou_threshold, projection,
                                                           box_extension, evaluation_metric, verbose)
        if save_path is not None:
            with open(save_path, "wb") as fh:         # (np.save(path) would append ".npy" to another suffix)
                np.save(fh, final_segmentation)
    return (results, final_segmentation) if return_segmentation else results


def _get_best_parameters_from_grid_search_combinations(result_dir, best_params_path, grid_search_values, evaluation_metric):
    """Reference :245-263."""
    if os.path.exists(best_params_path):
        print("The best parameters are already saved at:", best_params_path)
        return
    criterion = "mSA" if evaluation_metric == "sa" else "Dice"
    best_kwargs, best_metric = evaluate_instance_segmentation_grid_search(
        result_dir=result_dir, grid_search_parameters=list(grid_search_values.keys()), criterion=criterion)
    best_kwargs[criterion] = best_metric
    pd.DataFrame.from_dict([best_kwargs]).to_csv(best_params_path)
    print("Best grid-search result:", best_metric, "with parmeters:\n", ", ".join(f"{k} = {v}" for k, v in best_kwargs.items()))


def run_multi_dimensional_segmentation_grid_search(
    volume: np.ndarray, ground_truth: np.ndarray, model_type: str, checkpoint_path: Union[str, os.PathLike],
    embedding_path: Optional[Union[str, os.PathLike]], result_dir: Union[str, os.PathLike], interactive_seg_mode: str = "box",
    verbose: bool = False, grid_search_values: Optional[Dict[str, List]] = None, min_size: int = 0,
    evaluation_metric: Literal["sa", "dice"] = "sa", store_segmentation: bool = False,
    predictor=None, image_embeddings=None,
) -> str:
    """Reference ``run_multi_dimensional_segmentation_grid_search`` (:266-376): every combination of ``grid_search_values`` (three
    parameters of ``segment_slices_from_ground_truth``; default: ``default_grid_search_values_multi_dimensional_segmentation``) is run
    and scored; ``<result_dir>/all_grid_search_results.csv`` holds one row per combination and
    ``<result_dir>/grid_search_params_multi_dimensional_segmentation.csv`` the best one.  Returns the latter's path.  The model, the
    embeddings and the seeds in the middle slices are computed once for the whole grid."""
    if grid_search_values is None:
        grid_search_values = default_grid_search_values_multi_dimensional_segmentation()
    assert len(grid_search_values.keys()) == 3, "There must be three grid-search parameters. See above for details."
    os.makedirs(result_dir, exist_ok=True)
    result_path = os.path.join(result_dir, "all_grid_search_results.csv")
    best_params_path = os.path.join(result_dir, "grid_search_params_multi_dimensional_segmentation.csv")
    if os.path.exists(result_path):
        _get_best_parameters_from_grid_search_combinations(result_dir, best_params_path, grid_search_values, evaluation_metric)
        return best_params_path
    gs_combinations = [{k: v for k, v in zip(grid_search_values.keys(), vals)} for vals in product(*grid_search_values.values())]
    prediction_dir = os.path.join(result_dir, "predictions")
    os.makedirs(prediction_dir, exist_ok=True)
    assert volume.ndim == 3
    predictor, image_embeddings = _model_and_embeddings(volume, model_type, checkpoint_path, embedding_path, None, verbose, predictor,
                                                        image_embeddings)
    seeded = _seed_objects(ground_truth, predictor, image_embeddings, interactive_seg_mode, min_size, verbose)
    net_list = []
    for i, gs_kwargs in tqdm(enumerate(gs_combinations), total=len(gs_combinations),
                             desc="Run grid-search for multi-dimensional segmentation", disable=not verbose):
        results, segmentation = _propagate_and_score(seeded, ground_truth, predictor, image_embeddings,
                                                     evaluation_metric=evaluation_metric, verbose=verbose, **gs_kwargs)
        if store_segmentation:
            np.save(os.path.join(prediction_dir, f"grid_search_result_{i:05}.npy"), segmentation)
        net_list.append(pd.DataFrame([{**results, **gs_kwargs}]))
    pd.concat(net_list, ignore_index=True).to_csv(result_path)
    _get_best_parameters_from_grid_search_combinations(result_dir, best_params_path, grid_search_values, evaluation_metric)
    print("The best grid-search parameters have been computed and stored at:", best_params_path)
    return best_params_path
