"""Evaluation of segmentations (reference micro_sam/evaluation/): the elf metrics on the device scorer ``ops.label_matching``
(``evaluation``), the grid-search / inference drivers of the automatic instance segmentation (``instance_segmentation``), and the
prompt-based inference from ground truth (``inference``), whose public functions are also reachable from this package."""

_INFERENCE = ("precompute_all_embeddings", "precompute_all_prompts", "run_inference_with_prompts", "run_inference_with_iterative_prompting",
              "run_amg", "run_apg", "run_instance_segmentation_with_decoder")
__all__ = list(_INFERENCE)


def __getattr__(name):
    if name in _INFERENCE:                       # imported on first use: the submodule pulls in the predictor and the segmenters
        from . import inference
        return getattr(inference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
