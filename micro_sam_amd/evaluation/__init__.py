"""Evaluation of segmentations (reference micro_sam/evaluation/): the elf metrics on the device scorer ``ops.label_matching``
(``evaluation``), the grid-search / inference drivers of the automatic instance segmentation (``instance_segmentation``), and the
prompt-based inference from ground truth (``inference``) and the evaluation / grid search of the interactive 3-d segmentation
(``multi_dimensional_segmentation``); the public functions of the last two are also reachable from this package."""

_INFERENCE = ("precompute_all_embeddings", "precompute_all_prompts", "run_inference_with_prompts", "run_inference_with_iterative_prompting",
              "run_amg", "run_apg", "run_instance_segmentation_with_decoder")
_MULTI_DIMENSIONAL = ("default_grid_search_values_multi_dimensional_segmentation", "segment_slices_from_ground_truth",
                      "run_multi_dimensional_segmentation_grid_search")
__all__ = list(_INFERENCE) + list(_MULTI_DIMENSIONAL)


def __getattr__(name):
    if name in _INFERENCE:                       # imported on first use: the submodule pulls in the predictor and the segmenters
        from . import inference
        return getattr(inference, name)
    if name in _MULTI_DIMENSIONAL:
        from . import multi_dimensional_segmentation
        return getattr(multi_dimensional_segmentation, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
