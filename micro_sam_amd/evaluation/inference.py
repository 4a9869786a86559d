"""Inference with prompts derived from the ground truth (reference micro_sam/evaluation/inference.py): ``run_inference_with_prompts``,
``run_inference_with_iterative_prompting``, prompt pre-computation and caching, and the thin AMG / APG / AIS drivers, with the
reference's names, signatures, prompt rules and file layout (``points-p{P}-n{N}.pkl`` / ``boxes.pkl``, ``iteration{i:02}`` folders,
images whose outputs exist are skipped).

Where the work runs: the ground truth goes to the device ONCE per image; object ids, centres and bounding boxes come from one
``ops.label_props`` call (csrc/labelprops.hip) instead of skimage's regionprops and a host distance transform; for iterative prompting
the one-hot ground truth stays on the device for all iterations, so ``IterativePromptGenerator`` runs where the predicted masks are and
only the new [N, 2, 2] coordinates come back to the host per iteration.

Differences that follow from this environment, as in ``evaluation/instance_segmentation.py``: images and ground truth may be paths
(read with ``util.load_image_data``) or arrays (named ``image_{i}``), and predictions are written as ``<stem>.npy`` (imageio is not
vendored).  The object ids of an image are its positive labels (the reference takes ``np.unique(gt)[1:]``, which assumes a background)."""
from __future__ import annotations

import os
import pickle
from copy import deepcopy
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from tqdm import tqdm

from .. import ops, util
from ..inference import batched_inference
from ..instance_segmentation import (AutomaticMaskGenerator, AutomaticPromptGenerator, InstanceSegmentationWithDecoder,
                                     TiledAutomaticMaskGenerator, TiledInstanceSegmentationWithDecoder, get_predictor_and_decoder)
from ..predictor import SamPredictor
from ..prompt_generators import IterativePromptGenerator, PointAndBoxPromptGenerator
from . import instance_segmentation


def _load_prompts(cached_point_prompts, save_point_prompts, cached_box_prompts, save_box_prompts, image_name):
    """Reference :31-66: the prompts of ``image_name`` from the caches (a path is loaded on first use), or None when nothing is cached."""

    def load_prompt_type(cached_prompts, save_prompts):
        if cached_prompts is None or save_prompts:                       # we don't have cached prompts
            return cached_prompts, None
        if isinstance(cached_prompts, str):                              # cached, but not loaded yet
            with open(cached_prompts, "rb") as f:
                cached_prompts = pickle.load(f)
        return cached_prompts, cached_prompts[image_name]

    cached_point_prompts, point_prompts = load_prompt_type(cached_point_prompts, save_point_prompts)
    cached_box_prompts, box_prompts = load_prompt_type(cached_box_prompts, save_box_prompts)
    if point_prompts is None and box_prompts is None:
        return None, cached_point_prompts, cached_box_prompts
    input_point, input_label = ([], []) if point_prompts is None else point_prompts
    input_box = [] if box_prompts is None else box_prompts
    return (input_point, input_label, input_box), cached_point_prompts, cached_box_prompts


def _object_ids(gt_dev: torch.Tensor) -> torch.Tensor:
    ids = torch.unique(gt_dev)
    return ids[ids > 0].contiguous()


def _get_batched_prompts(gt, gt_ids, use_points, use_boxes, n_positives, n_negatives, dilation):
    """Reference :69-93.  ``gt``: the label image (numpy, or an int32 tensor already on the device); ``gt_ids``: sorted object ids
    (array or device tensor).  Centres and boxes of the objects come from ``ops.label_props``.  Boxes alone, or one positive point at
    the centre, are written straight from them - what ``PointAndBoxPromptGenerator`` returns for these settings, without the one-hot
    masks; every other setting samples pixels and goes through the generator on the host, as in the reference."""
    gt_dev = util._labels_on_device(gt)
    ids_dev = gt_ids if torch.is_tensor(gt_ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(gt_ids).astype(np.int32)))
    ids_dev = ids_dev.to(device=gt_dev.device, dtype=torch.int32).contiguous()
    prompt_generator = PointAndBoxPromptGenerator(n_positive_points=n_positives, n_negative_points=n_negatives, dilation_strength=dilation,
                                                  get_point_prompts=use_points, get_box_prompts=use_boxes)
    center_only = (not use_points) or (n_positives == 1 and n_negatives == 0)
    props = ops.label_props(gt_dev, ids_dev, centers=bool(use_points))
    if int(ids_dev.numel()) and int(props.area.min()) == 0:
        raise KeyError("gt_ids holds an id that is not in the ground truth")
    bbox = props.bbox.cpu().numpy()
    center = props.center.cpu().numpy() if use_points else None
    if center_only:
        points = np.ascontiguousarray(center[:, None, ::-1], dtype=np.float32) if use_points else None           # (x, y)
        point_labels = np.ones((len(bbox), 1), np.float32) if use_points else None
        boxes = np.ascontiguousarray(bbox[:, [1, 0, 3, 2]], dtype=np.float32) if use_boxes else None             # xyxy
        return points, point_labels, boxes
    masks = util.segmentation_to_one_hot(gt_dev.to(torch.int64), ids_dev).cpu()
    points, point_labels, boxes, _ = prompt_generator(masks, [tuple(b) for b in bbox.tolist()], [tuple(c) for c in center.tolist()])

    def to_numpy(x):
        return x if x is None else x.numpy()

    return to_numpy(points), to_numpy(point_labels), to_numpy(boxes)


def _run_inference_with_prompts_for_image(predictor, image, gt, use_points, use_boxes, n_positives, n_negatives, dilation, batch_size,
                                          cached_prompts, embedding_path):
    """Reference :96-132: -> (instance label image, (points, point_labels, boxes))."""
    if cached_prompts is None:
        gt_dev = util._labels_on_device(gt)
        points, point_labels, boxes = _get_batched_prompts(gt_dev, _object_ids(gt_dev), use_points, use_boxes, n_positives, n_negatives,
                                                           dilation)
    else:
        points, point_labels, boxes = cached_prompts
    prompts = deepcopy((points, point_labels, boxes))
    # multi-masking only for a single positive point without box
    multimasking = (not use_boxes) and (n_positives == 1 and n_negatives == 0)
    instance_labels = batched_inference(predictor, image, batch_size, boxes=boxes, points=points, point_labels=point_labels,
                                        multimasking=multimasking, embedding_path=embedding_path, return_instance_segmentation=True)
    return instance_labels, prompts


def _named(item, i: int) -> Tuple[str, bool]:
    return instance_segmentation._named(item, i)


def _read(item) -> np.ndarray:
    if isinstance(item, np.ndarray):
        return item
    assert os.path.exists(item), item
    return np.asarray(util.load_image_data(item))


def _read_gt(item) -> np.ndarray:
    """The ground truth relabelled sequentially (reference: ``relabel_sequential(imread(gt_path).astype("uint32"))[0]``)."""
    gt = _read(item).astype("uint32")
    values, inverse = np.unique(gt, return_inverse=True)
    new = np.arange(len(values), dtype=np.uint32) + (0 if len(values) and values[0] == 0 else 1)
    return new[inverse].reshape(gt.shape)


def precompute_all_embeddings(predictor: SamPredictor, image_paths: List[Union[str, os.PathLike, np.ndarray]],
                              embedding_dir: Union[str, os.PathLike]) -> None:
    """Reference :135-151: the embeddings of all images, saved as ``<embedding_dir>/<name>.zarr``."""
    for i, image_path in enumerate(tqdm(image_paths, desc="Precompute embeddings")):
        image_name, _ = _named(image_path, i)
        util.precompute_image_embeddings(predictor, _read(image_path), os.path.join(embedding_dir, f"{image_name}.zarr"), ndim=2)


def _precompute_prompts(gt_path, use_points, use_boxes, n_positives, n_negatives, dilation, name=None):
    name = os.path.basename(gt_path) if name is None else name
    gt_dev = util._labels_on_device(_read_gt(gt_path))
    input_point, input_label, input_box = _get_batched_prompts(gt_dev, _object_ids(gt_dev), use_points, use_boxes, n_positives, n_negatives,
                                                               dilation)
    if use_boxes and not use_points:
        return name, input_box
    return name, (input_point, input_label)


def _label_name(gt_path, i: int) -> str:
    return f"image_{i}" if isinstance(gt_path, np.ndarray) else os.path.basename(gt_path)


def precompute_all_prompts(gt_paths: List[Union[str, os.PathLike, np.ndarray]], prompt_save_dir: Union[str, os.PathLike],
                           prompt_settings: List[Dict[str, Any]]) -> None:
    """Reference :170-214: for every setting ({"use_points", "use_boxes", "n_positives", "n_negatives", optional "dilation"}) the
    prompts of all ground-truth images, pickled as ``boxes.pkl`` or ``points-p{P}-n{N}.pkl``; existing files are kept."""
    os.makedirs(prompt_save_dir, exist_ok=True)
    for settings in tqdm(prompt_settings, desc="Precompute prompts"):
        use_points, use_boxes = settings["use_points"], settings["use_boxes"]
        n_positives, n_negatives = settings["n_positives"], settings["n_negatives"]
        dilation = settings.get("dilation", 5)
        if use_boxes and not use_points:
            prompt_save_path = os.path.join(prompt_save_dir, "boxes.pkl")
        else:
            prompt_save_path = os.path.join(prompt_save_dir, f"points-p{n_positives}-n{n_negatives}.pkl")
        if os.path.exists(prompt_save_path):
            continue
        results = [_precompute_prompts(gt_path, use_points=use_points, use_boxes=use_boxes, n_positives=n_positives, n_negatives=n_negatives,
                                       dilation=dilation, name=_label_name(gt_path, i))
                   for i, gt_path in enumerate(tqdm(gt_paths, desc=f"Precompute prompts for p{n_positives}-n{n_negatives}"))]
        with open(prompt_save_path, "wb") as f:
            pickle.dump({res[0]: res[1] for res in results}, f)


def _get_prompt_caching(prompt_save_dir, use_points, use_boxes, n_positives, n_negatives):
    """Reference :217-252."""

    def get_prompt_type_caching(use_type, save_name):
        if not use_type:
            return None, False, None
        prompt_save_path = os.path.join(prompt_save_dir, save_name)
        if os.path.exists(prompt_save_path):
            print("Using precomputed prompts from", prompt_save_path)
            return prompt_save_path, False, prompt_save_path             # loaded when first needed
        print("Saving prompts in", prompt_save_path)
        return {}, True, prompt_save_path

    if prompt_save_dir is None:
        print("Prompts are not cached.")
        return None, False, None, None, False, None
    return (*get_prompt_type_caching(use_points, f"points-p{n_positives}-n{n_negatives}.pkl"),
            *get_prompt_type_caching(use_boxes, "boxes.pkl"))


def run_inference_with_prompts(predictor: SamPredictor, image_paths: List[Union[str, os.PathLike, np.ndarray]],
                               gt_paths: List[Union[str, os.PathLike, np.ndarray]], embedding_dir: Union[str, os.PathLike],
                               prediction_dir: Union[str, os.PathLike], use_points: bool, use_boxes: bool, n_positives: int,
                               n_negatives: int, dilation: int = 5, prompt_save_dir: Optional[Union[str, os.PathLike]] = None,
                               batch_size: int = 512) -> None:
    """Reference :255-344: segment every image from prompts derived from its ground truth; one label image per image in
    ``prediction_dir``.  With ``prompt_save_dir`` the prompts are read from / written to the pickles of ``precompute_all_prompts``."""
    if not (use_points or use_boxes):
        raise ValueError("You need to use at least one of point or box prompts.")
    if len(image_paths) != len(gt_paths):
        raise ValueError(f"Expect same number of images and gt images, got {len(image_paths)}, {len(gt_paths)}")
    (cached_point_prompts, save_point_prompts, point_prompt_save_path,
     cached_box_prompts, save_box_prompts, box_prompt_save_path) = _get_prompt_caching(prompt_save_dir, use_points, use_boxes, n_positives,
                                                                                       n_negatives)
    os.makedirs(prediction_dir, exist_ok=True)
    if prompt_save_dir is not None:
        os.makedirs(prompt_save_dir, exist_ok=True)
    for i, (image_path, gt_path) in enumerate(tqdm(zip(image_paths, gt_paths), total=len(image_paths), desc="Run inference with prompts")):
        image_name, _ = _named(image_path, i)
        label_name = _label_name(gt_path, i)
        prediction_path = os.path.join(prediction_dir, f"{image_name}.npy")
        if os.path.exists(prediction_path):
            continue
        im, gt = _read(image_path), _read_gt(gt_path)
        embedding_path = None if embedding_dir is None else os.path.join(embedding_dir, f"{image_name}.zarr")
        this_prompts, cached_point_prompts, cached_box_prompts = _load_prompts(cached_point_prompts, save_point_prompts, cached_box_prompts,
                                                                               save_box_prompts, label_name)
        instances, this_prompts = _run_inference_with_prompts_for_image(
            predictor, im, gt, n_positives=n_positives, n_negatives=n_negatives, dilation=dilation, use_points=use_points,
            use_boxes=use_boxes, batch_size=batch_size, cached_prompts=this_prompts, embedding_path=embedding_path)
        if save_point_prompts:
            cached_point_prompts[label_name] = this_prompts[:2]
        if save_box_prompts:
            cached_box_prompts[label_name] = this_prompts[-1]
        np.save(prediction_path, np.asarray(instances))
    if save_point_prompts:
        with open(point_prompt_save_path, "wb") as f:
            pickle.dump(cached_point_prompts, f)
    if save_box_prompts:
        with open(box_prompt_save_path, "wb") as f:
            pickle.dump(cached_box_prompts, f)


def _save_segmentation(masks, prediction_path):
    """Reference :347-352: object masks [N, 1, H, W] -> one label image (``util.mask_data_to_segmentation``), saved."""
    areas = masks.flatten(1).sum(dim=1).cpu().numpy()
    masks = masks.squeeze(1).to(torch.bool).cpu().numpy()
    records = [{"segmentation": mask, "area": area} for mask, area in zip(masks, areas)]
    np.save(prediction_path, util.mask_data_to_segmentation(records))


def _get_batched_iterative_prompts(sampled_binary_gt, masks, batch_size, prompt_generator):
    """Reference :355-372."""
    n_samples = sampled_binary_gt.shape[0]
    n_batches = int(np.ceil(float(n_samples) / batch_size))
    next_coords, next_labels = [], []
    for batch_idx in range(n_batches):
        batch_start, batch_stop = batch_idx * batch_size, min((batch_idx + 1) * batch_size, n_samples)
        batch_coords, batch_labels, _, _ = prompt_generator(sampled_binary_gt[batch_start:batch_stop], masks[batch_start:batch_stop])
        next_coords.append(batch_coords)
        next_labels.append(batch_labels)
    return torch.concatenate(next_coords), torch.concatenate(next_labels)


@torch.no_grad()
def _run_inference_with_iterative_prompting_for_image(predictor, image, gt, start_with_box_prompt, dilation, batch_size, embedding_path,
                                                      n_iterations, prediction_paths, use_masks=False):
    """Reference :375-459.  The ground truth is uploaded once; its one-hot form stays on the device for all iterations.  Returns the
    point prompts of the last round, (points [N, P, 2], point_labels [N, P]) (the reference returns nothing)."""
    verbose_embeddings = False
    prompt_generator = IterativePromptGenerator()
    gt_dev = util._labels_on_device(gt)
    gt_ids = _object_ids(gt_dev)
    # multi-masking only for a single positive point without box
    if start_with_box_prompt:
        use_boxes, use_points, n_positives, multimasking = True, False, 0, False
    else:
        use_boxes, use_points, n_positives, multimasking = False, True, 1, True
    points, point_labels, boxes = _get_batched_prompts(gt_dev, gt_ids, use_points=use_points, use_boxes=use_boxes, n_positives=n_positives,
                                                       n_negatives=0, dilation=dilation)
    sampled_binary_gt = util.segmentation_to_one_hot(gt_dev.to(torch.int64), gt_ids)       # [N, 1, H, W] on the device
    logits_masks = None
    for iteration in range(n_iterations):
        if iteration == 0 or not use_masks:                               # no logits for the first iteration, or when not desired
            logits_masks = None
        batched_outputs = batched_inference(
            predictor=predictor, image=image, batch_size=batch_size, boxes=boxes, points=points, point_labels=point_labels,
            multimasking=multimasking, embedding_path=embedding_path, return_instance_segmentation=False, logits_masks=logits_masks,
            verbose_embeddings=verbose_embeddings)
        multimasking = False                                              # later iterations carry several prompts per object
        masks = torch.stack([m["segmentation"][None] for m in batched_outputs]).to(torch.float32)
        next_coords, next_labels = _get_batched_iterative_prompts(sampled_binary_gt, masks, batch_size, prompt_generator)
        next_coords, next_labels = next_coords.detach().cpu().numpy(), next_labels.detach().cpu().numpy()
        points = next_coords if points is None else np.concatenate([points, next_coords], axis=1)
        point_labels = next_labels if point_labels is None else np.concatenate([point_labels, next_labels], axis=1)
        if use_masks:
            logits_masks = torch.stack([m["logits"] for m in batched_outputs])
        _save_segmentation(masks, prediction_paths[iteration])
    return points, point_labels


def run_inference_with_iterative_prompting(predictor: SamPredictor, image_paths: List[Union[str, os.PathLike, np.ndarray]],
                                           gt_paths: List[Union[str, os.PathLike, np.ndarray]], embedding_dir: Union[str, os.PathLike],
                                           prediction_dir: Union[str, os.PathLike], start_with_box_prompt: bool = True, dilation: int = 5,
                                           batch_size: int = 32, n_iterations: int = 8, use_masks: bool = False) -> None:
    """Reference :462-527: per image, ``n_iterations`` rounds of prompting - a box or the centre point first, then one positive and
    one negative point per object and round where prediction and ground truth disagree; the segmentation of round i is written to
    ``<prediction_dir>/iteration{i:02}``.  ``use_masks`` feeds the logits of the previous round back to the model."""
    if len(image_paths) != len(gt_paths):
        raise ValueError(f"Expect same number of images and gt images, got {len(image_paths)}, {len(gt_paths)}")
    for i in range(n_iterations):
        os.makedirs(os.path.join(prediction_dir, f"iteration{i:02}"), exist_ok=True)
    if use_masks:
        print("The iterative prompting will make use of logits masks from previous iterations.")
    for i, (image_path, gt_path) in enumerate(tqdm(zip(image_paths, gt_paths), total=len(image_paths),
                                                   desc="Run inference with iterative prompting for all images")):
        image_name, _ = _named(image_path, i)
        prediction_paths = [os.path.join(prediction_dir, f"iteration{k:02}", f"{image_name}.npy") for k in range(n_iterations)]
        if all(os.path.exists(prediction_path) for prediction_path in prediction_paths):
            continue
        image, gt = _read(image_path), _read_gt(gt_path)
        embedding_path = None if embedding_dir is None else os.path.join(embedding_dir, f"{image_name}.zarr")
        _run_inference_with_iterative_prompting_for_image(
            predictor, image, gt, start_with_box_prompt=start_with_box_prompt, dilation=dilation, batch_size=batch_size,
            embedding_path=embedding_path, n_iterations=n_iterations, prediction_paths=prediction_paths, use_masks=use_masks)


# ------------------------------------------------------------------------------------------------- automatic segmentation drivers

def _experiment_folders(experiment_folder, prefix: str, cache_embeddings: bool):
    embedding_folder = None
    if cache_embeddings:
        embedding_folder = os.path.join(experiment_folder, "embeddings")
        os.makedirs(embedding_folder, exist_ok=True)
    prediction_folder = os.path.join(experiment_folder, prefix, "inference")
    gs_result_folder = os.path.join(experiment_folder, prefix, "grid_search")
    os.makedirs(prediction_folder, exist_ok=True)
    os.makedirs(gs_result_folder, exist_ok=True)
    return embedding_folder, prediction_folder, gs_result_folder


def _check_tiling(tiling_window_params) -> bool:
    if not tiling_window_params:
        return False
    if not isinstance(tiling_window_params, dict):
        raise RuntimeError("The tiling window parameters are expected to be provided as a dictionary of params.")
    if "tile_shape" not in tiling_window_params:
        raise RuntimeError("'tile_shape' parameter is missing from the provided parameters.")
    if "halo" not in tiling_window_params:
        raise RuntimeError("'halo' parameter is missing from the provided parameters.")
    return True


def _grid_search_and_inference(segmenter, grid_search_values, prefix, experiment_folder, val_image_paths, val_gt_paths, test_image_paths,
                               cache_embeddings, tiling_window_params) -> str:
    embedding_folder, prediction_folder, gs_result_folder = _experiment_folders(experiment_folder, prefix, cache_embeddings)
    instance_segmentation.run_instance_segmentation_grid_search_and_inference(
        segmenter=segmenter, grid_search_values=grid_search_values, val_image_paths=val_image_paths, val_gt_paths=val_gt_paths,
        test_image_paths=test_image_paths, embedding_dir=embedding_folder, prediction_dir=prediction_folder, result_dir=gs_result_folder,
        experiment_folder=experiment_folder, tiling_window_params=tiling_window_params)
    return prediction_folder


def run_amg(checkpoint: Union[str, os.PathLike], model_type: str, experiment_folder: Union[str, os.PathLike],
            val_image_paths: List[Union[str, os.PathLike]], val_gt_paths: List[Union[str, os.PathLike]],
            test_image_paths: List[Union[str, os.PathLike]], iou_thresh_values: Optional[List[float]] = None,
            stability_score_values: Optional[List[float]] = None, peft_kwargs: Optional[Dict] = None, cache_embeddings: bool = False,
            tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None) -> str:
    """Reference ``run_amg`` (:535-618): grid search of the AMG thresholds on the validation images, inference with the best setting
    on the test images; returns the folder of the predictions (``<experiment_folder>/amg/inference``)."""
    predictor = util.get_sam_model(model_type=model_type, checkpoint_path=checkpoint, peft_kwargs=peft_kwargs)
    amg = (TiledAutomaticMaskGenerator if _check_tiling(tiling_window_params) else AutomaticMaskGenerator)(predictor)
    grid_search_values = instance_segmentation.default_grid_search_values_amg(iou_thresh_values=iou_thresh_values,
                                                                              stability_score_values=stability_score_values)
    return _grid_search_and_inference(amg, grid_search_values, "amg", experiment_folder, val_image_paths, val_gt_paths, test_image_paths,
                                      cache_embeddings, tiling_window_params)


def run_apg(checkpoint: Optional[Union[str, os.PathLike]], model_type: str, experiment_folder: Union[str, os.PathLike],
            val_image_paths: List[Union[str, os.PathLike]], val_gt_paths: List[Union[str, os.PathLike]],
            test_image_paths: List[Union[str, os.PathLike]], peft_kwargs: Optional[Dict] = None, cache_embeddings: bool = False,
            tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None) -> str:
    """Reference ``run_apg`` (:621-681); tiling is not implemented there either."""
    predictor, decoder = get_predictor_and_decoder(model_type=model_type, checkpoint_path=checkpoint, peft_kwargs=peft_kwargs)
    if tiling_window_params:
        raise NotImplementedError
    segmenter = AutomaticPromptGenerator(predictor, decoder)
    return _grid_search_and_inference(segmenter, instance_segmentation.default_grid_search_values_apg(), "apg", experiment_folder,
                                      val_image_paths, val_gt_paths, test_image_paths, cache_embeddings, tiling_window_params)


def run_instance_segmentation_with_decoder(checkpoint: Union[str, os.PathLike], model_type: str, experiment_folder: Union[str, os.PathLike],
                                           val_image_paths: List[Union[str, os.PathLike]], val_gt_paths: List[Union[str, os.PathLike]],
                                           test_image_paths: List[Union[str, os.PathLike]], peft_kwargs: Optional[Dict] = None,
                                           cache_embeddings: bool = False,
                                           tiling_window_params: Optional[Dict[str, Tuple[int, int]]] = None) -> str:
    """Reference ``run_instance_segmentation_with_decoder`` (:689-768)."""
    predictor, decoder = get_predictor_and_decoder(model_type=model_type, checkpoint_path=checkpoint, peft_kwargs=peft_kwargs)
    ais_class = TiledInstanceSegmentationWithDecoder if _check_tiling(tiling_window_params) else InstanceSegmentationWithDecoder
    return _grid_search_and_inference(ais_class(predictor, decoder), instance_segmentation.default_grid_search_values_instance_segmentation_with_decoder(),
                                      "instance_segmentation_with_decoder", experiment_folder, val_image_paths, val_gt_paths, test_image_paths,
                                      cache_embeddings, tiling_window_params)
