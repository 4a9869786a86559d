"""Evaluation of segmentations (reference micro_sam/evaluation/): the elf metrics on the device scorer ``ops.label_matching``
(``evaluation``), and the grid-search / inference drivers of the automatic instance segmentation (``instance_segmentation``)."""
