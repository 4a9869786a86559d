"""``SemanticSamTrainer``, ``SemanticMapsSamTrainer`` and ``CustomDiceLoss`` (reference ``micro_sam/training/semantic_sam_trainer.py``):
fine-tuning SAM for multi-class semantic segmentation.  The recipe has no prompts: every image is decoded once with
``multimask_output=True``, the three full-resolution masks are the logits of three classes, and the loss is the soft-max dice loss plus the
cross-entropy against the label image.

Both parts of the loss come from ONE fused call on the device (``training.functional.semantic_loss``, csrc/semloss.hip: two launches
forward, one backward) instead of the reference's tree of torch operators (soft-max, a per-class ``==`` and ``cat``, three products, three
reductions, ``log_softmax``, ``nll_loss`` and the backward of each).  ``CustomDiceLoss`` restates the reference's class on torch_em's
``DiceLoss()``.  PARITY UNPINNED: torch_em is neither vendored in the reference nor installed here; the loss follows its published source,
with the same standing as ``joint_sam_trainer.DiceBasedDistanceLoss``.  Two deliberate differences from torch
(DESIGN.md 8.6): a class id outside [0, num_classes) is ignored by the cross-entropy like -100 (torch: a device-side assert), and a batch
without any valid pixel has a cross-entropy of 0 (torch: NaN).

Like ``SamTrainer`` there is no torch_em base class: the train step is ``SamTrainer._optimization_pass`` (so the data-parallel gradient
exchange is the same), ``fit`` the plain loop, ``validate`` the reference's ``_validate_impl``.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Iterable, Optional

import torch
from torch import nn

from . import functional as HF
from .sam_trainer import SamTrainer


def _fold_depth(pred: torch.Tensor, target: torch.Tensor):
    """Volumes (``models.sam_3d_wrapper.Sam3DWrapper``): prediction [B, C, D, H, W] with target [B, 1, D, H, W] or [B, D, H, W] ->
    [B, C, D H, W] and [B, D H, W].  Exact for this loss: the dice sums and the cross-entropy mean run over batch and space per class,
    so it does not matter which spatial axis a pixel lies on.  Anything else passes through."""
    if pred.dim() != 5:
        return pred, target
    b, c, d, h, w = pred.shape
    if tuple(target.shape) not in ((b, 1, d, h, w), (b, d, h, w)):
        raise ValueError(f"the target of a prediction {tuple(pred.shape)} must be {(b, 1, d, h, w)} or {(b, d, h, w)}, got {tuple(target.shape)}")
    return pred.reshape(b, c, d * h, w), target.reshape(b, d * h, w)


class CustomDiceLoss(nn.Module):
    """The reference's ``CustomDiceLoss``: dice over one-hot labels.  prediction [B, num_classes, H, W], target [B, 1, H, W] (or
    [B, H, W]) class ids -> torch_em ``DiceLoss()`` of the (soft-max of the) prediction against the one-hot target, summed over the
    classes.  One fused device call with ``ce_weight=0``.  Volumes, prediction [B, num_classes, D, H, W] with target [B, 1, D, H, W] or
    [B, D, H, W], are folded to images first (``_fold_depth``)."""

    def __init__(self, num_classes: int, softmax: bool = True) -> None:
        super().__init__()
        self.num_classes = int(num_classes)
        self.softmax = bool(softmax)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        pred, target = _fold_depth(pred, target)
        if pred.dim() != 4 or pred.shape[1] != self.num_classes:
            raise ValueError(f"CustomDiceLoss: the prediction must be [B, {self.num_classes}, H, W], got {tuple(pred.shape)}")
        return HF.semantic_loss(pred, target, dice_weight=1.0, ce_weight=0.0, softmax=self.softmax)[0]


class SemanticSamTrainer(SamTrainer):
    """Reference ``SemanticSamTrainer(convert_inputs, num_classes, dice_weight=None, **kwargs)``.  ``kwargs``: ``model`` (a
    ``TrainableSAM``), ``optimizer``, optionally ``loss`` / ``metric`` (callables (prediction, target) -> scalar; default
    ``CustomDiceLoss(num_classes)``) and ``device``.  With the default loss ``_compute_loss`` is one fused call; with a ``loss=`` of the
    user's it is the reference's two terms, that loss plus torch's ``nn.CrossEntropyLoss``.  ``dice_weight=None``: dice + ce, otherwise
    ``dice_weight * dice + (1 - dice_weight) * ce``."""

    def __init__(self, convert_inputs: Callable, num_classes: int, dice_weight: Optional[float] = None, **kwargs) -> None:
        unknown = sorted(set(kwargs) - {"model", "optimizer", "loss", "metric", "device"})
        if unknown or "model" not in kwargs or "optimizer" not in kwargs:
            raise TypeError(f"SemanticSamTrainer takes model=, optimizer= and optionally loss=, metric=, device= (there is no torch_em "
                            f"base class here); got {sorted(kwargs)}")
        model, optimizer = kwargs["model"], kwargs["optimizer"]
        loss, metric, device = kwargs.get("loss"), kwargs.get("metric"), kwargs.get("device")
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes <= 1:
            raise ValueError(f"SemanticSamTrainer: num_classes must be an integer above 1 (the background is a class), got {num_classes!r}")
        if dice_weight is not None and (dice_weight < 0 or dice_weight > 1):
            raise ValueError("The weight factor should lie between 0 and 1.")
        super().__init__(model=model, optimizer=optimizer, convert_inputs=convert_inputs, n_sub_iteration=1, device=device)
        self._fused = loss is None
        self.loss = CustomDiceLoss(num_classes=num_classes) if loss is None else loss
        self.metric = CustomDiceLoss(num_classes=num_classes) if metric is None else metric
        self.num_classes = num_classes
        self.compute_ce_loss = nn.CrossEntropyLoss()
        self.dice_weight = dice_weight
        self.last_parts = None                                          # (dice, ce) of the last ``_compute_loss``: 0-dim device tensors
        self.last_metric = None                                         # 1 - metric / num_classes of the last ``validate``

    def _weights(self):
        return (1.0, 1.0) if self.dice_weight is None else (float(self.dice_weight), 1.0 - float(self.dice_weight))

    # ---- reference :78-93
    def _compute_loss(self, y, masks):
        """The combined (weighted) dice and cross-entropy loss between the prediction [B, num_classes, H, W] and the target
        [B, 1, H, W] (class ids); for a volumetric model [B, num_classes, D, H, W] and [B, 1, D, H, W] or [B, D, H, W], folded to
        images first (``_fold_depth``)."""
        masks, y = _fold_depth(masks, y)
        if masks.dim() != 4 or masks.shape[1] != self.num_classes:
            raise ValueError(f"SemanticSamTrainer: the model gives {masks.shape[1] if masks.dim() == 4 else tuple(masks.shape)} channels for "
                             f"num_classes = {self.num_classes} (TrainableSAM with multimask_output=True gives 3)")
        target = y.to(self.device, non_blocking=True)
        wd, wc = self._weights()
        if self._fused:
            net_loss, stats = HF.semantic_loss(masks, target, dice_weight=wd, ce_weight=wc, softmax=True)
            self.last_parts = (stats.dice, stats.ce)
            return net_loss
        dice_loss = self.loss(masks, target)
        ce_loss = self.compute_ce_loss(masks, target.squeeze(1).long())
        self.last_parts = (dice_loss.detach(), ce_loss.detach())
        return wd * dice_loss + wc * ce_loss

    # ---- reference :95-111
    def _get_model_outputs(self, batched_inputs):
        if hasattr(self.model, "image_embeddings_oft"):
            image_embeddings, batched_inputs = self.model.image_embeddings_oft(batched_inputs)
            batched_outputs = self.model(batched_inputs, image_embeddings, multimask_output=True)
        else:       # the embeddings are computed as part of the forward pass
            batched_inputs = [{"image": inp["image"].to(self.device, non_blocking=True), "original_size": inp["original_size"]}
                              for inp in batched_inputs]
            batched_outputs = self.model(batched_inputs, multimask_output=True)
        return torch.stack([output["masks"].squeeze(0) for output in batched_outputs])

    def _semantic_iteration(self, x, y):
        masks = self._get_model_outputs(self.convert_inputs(x, y))
        return (self._compute_loss(y, masks),)

    # ---- reference :113-141
    def train_iteration(self, x, y) -> dict:
        self.model.train()
        (loss,), reduced = self._optimization_pass(lambda: self._semantic_iteration(x, y))
        dice_loss, ce_loss = self.last_parts if self.last_parts is not None else (float("nan"), float("nan"))
        rec = {"iteration": self._iteration, "loss": float(loss.detach()), "dice_loss": float(dice_loss), "ce_loss": float(ce_loss),
               "allreduce_bytes": reduced}
        self.history.append(rec)
        self._iteration += 1
        return rec

    # ---- reference :143-170
    @torch.no_grad()
    def validate(self, loader: Iterable) -> float:
        """The reference's validation metric: the net loss averaged over the loader.  ``last_metric`` then holds the score the reference
        prints, 1 - metric / num_classes."""
        self.model.eval()
        total, n = 0.0, 0
        for x, y in loader:
            total += float(self._semantic_iteration(x, y)[0])
            n += 1
        if n == 0:
            raise ValueError("SemanticSamTrainer.validate: the loader is empty")
        metric_val = total / n
        self.last_metric = 1 - metric_val / self.num_classes
        return metric_val

    def save_checkpoint(self, path: str, **extra_save_dict) -> None:
        """``model_state`` (the ``TrainableSAM``: keys ``sam.*``), the optimizer's state and the iteration - plain tensors and numbers, so
        that the file loads with ``weights_only=True``."""
        model_state = OrderedDict((k, v.detach().cpu()) for k, v in self.model.state_dict().items())
        torch.save({"model_state": model_state, "optimizer_state": self.optimizer.state_dict(), "iteration": self._iteration,
                    "num_classes": self.num_classes, **extra_save_dict}, path)

    def load_checkpoint(self, path: str) -> dict:
        save_dict = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(save_dict["model_state"])
        self.optimizer.load_state_dict(save_dict["optimizer_state"])
        self._iteration = int(save_dict["iteration"])
        return save_dict


class SemanticMapsSamTrainer(SemanticSamTrainer):
    """Reference ``SemanticMapsSamTrainer``: the loss alone, called as ``loss(target, masks)``."""

    def _compute_loss(self, y, masks):
        target = y.to(self.device, non_blocking=True)
        self.last_parts = None
        return self.loss(target, masks)
