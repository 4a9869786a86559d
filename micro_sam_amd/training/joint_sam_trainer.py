"""``JointSamTrainer`` (reference ``micro_sam/training/joint_sam_trainer.py:16-180``): SAM's interactive segmentation and the convolutional
(UNETR) decoder of the automatic instance segmentation trained together - the recipe behind ``train_sam(with_segmentation_decoder=True)``.
Every iteration makes two optimisation passes over one optimizer that holds the parameters of both: the iterative-prompting loss of
``SamTrainer``, then the decoder's loss against the foreground / centre-distance / boundary-distance targets.  Its checkpoints carry a
``decoder_state`` next to the ``model_state``, which is what ``instance_segmentation.get_predictor_and_decoder`` loads.

``DiceBasedDistanceLoss`` restates ``torch_em.loss.DiceBasedDistanceLoss`` (``DistanceLoss`` with dice for all three channels).  PARITY
UNPINNED: torch_em is neither vendored in the reference nor installed here; the loss follows its published source, with the same
standing as ``models/unetr.py`` and ``training/label_transform.py``.

The targets: a loader may deliver the reference's four channels ``[instances, foreground, centre, boundary]`` (made by torch_em's label
transform in its workers) or the raw instance labels as ONE channel; the trainer then makes the targets itself, per image, on the device
(``label_transform.PerObjectDistanceTransform``).

The UNETR half is a tree of torch operators on autograd (a HIP backward for it does not exist); the gradients of the library's convolutions
decide whether two runs of it agree bit for bit, which is not claimed (DESIGN.md 8.4 records what was observed).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Iterable, Optional

import torch
from torch import nn

from .label_transform import PerObjectDistanceTransform
from .sam_trainer import SamTrainer, dice_loss_per_channel


class DiceBasedDistanceLoss(nn.Module):
    """torch_em's ``DiceBasedDistanceLoss`` (unpinned): prediction and target ``[B, 3, H, W]`` = foreground, centre distance, boundary
    distance; the dice loss of the foreground channel plus the dice losses of the two distance channels.  With ``mask_distances_in_bg``
    prediction and target of the distance channels are both multiplied by the foreground TARGET, so the background (where the target holds
    the transform's fill value) does not count."""

    def __init__(self, mask_distances_in_bg: bool = True) -> None:
        super().__init__()
        self.mask_distances_in_bg = bool(mask_distances_in_bg)

    def forward(self, input_: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if input_.shape != target.shape or input_.dim() < 3 or input_.shape[1] != 3:
            raise ValueError(f"DiceBasedDistanceLoss: prediction and target must agree and have 3 channels, got {tuple(input_.shape)} and "
                             f"{tuple(target.shape)}")
        fg_target = target[:, 0:1]
        loss = dice_loss_per_channel(input_[:, 0:1], fg_target).sum()
        for c in (1, 2):
            p, t = input_[:, c:c + 1], target[:, c:c + 1]
            if self.mask_distances_in_bg:
                p, t = p * fg_target, t * fg_target
            loss = loss + dice_loss_per_channel(p, t).sum()
        return loss


class JointSamTrainer(SamTrainer):
    """``SamTrainer`` plus the decoder.  ``unetr``: ``models.unetr.get_unetr(sam.image_encoder)`` - it shares the image encoder with the
    SAM being trained; the optimizer must hold the parameters of both (the encoder's once).  ``instance_loss`` / ``instance_metric``:
    callables (prediction, target) -> scalar, by default ``DiceBasedDistanceLoss(mask_distances_in_bg=True)`` as in the reference's
    ``train_sam``.  ``label_transform``: what turns one-channel instance labels into the four channels, by default
    ``PerObjectDistanceTransform(instances=True, min_size=25)`` (the reference's ``default_sam_dataset``).  The other arguments are
    ``SamTrainer``'s."""

    def __init__(self, unetr: nn.Module, instance_loss: Optional[Callable] = None, instance_metric: Optional[Callable] = None,
                 label_transform: Optional[Callable] = None, **kwargs) -> None:
        super().__init__(**kwargs)
        self.unetr = unetr
        self.instance_loss = DiceBasedDistanceLoss(mask_distances_in_bg=True) if instance_loss is None else instance_loss
        self.instance_metric = DiceBasedDistanceLoss(mask_distances_in_bg=True) if instance_metric is None else instance_metric
        self.label_transform = PerObjectDistanceTransform(instances=True, min_size=25) if label_transform is None else label_transform

    # ---- the targets
    def _split_targets(self, y: torch.Tensor):
        """y [B, 4, H, W] (the reference's layout) or [B, 1, H, W] (raw instance labels) -> (instance labels [B, 1, H, W] on the host, as
        ``convert_inputs`` reads them; decoder targets float32 [B, 3, H, W] on the device)."""
        if y.dim() != 4 or y.shape[1] not in (1, 4):
            raise ValueError(f"JointSamTrainer: y must be [B, 4, H, W] (instances, foreground, centre, boundary) or [B, 1, H, W] (instance "
                             f"labels), got {tuple(y.shape)}")
        if y.shape[1] == 1:
            # per image on the device; a label transform that downloads for its connected components says so
            y = torch.stack([torch.as_tensor(self.label_transform(lab[0].to(self.device))) for lab in y])
            if y.shape[1] != 4:
                raise ValueError(f"JointSamTrainer: label_transform must return [instances, foreground, centre, boundary], got {y.shape[1]} channels")
        return y[:, 0:1].cpu(), y[:, 1:].to(self.device, dtype=torch.float32)

    # ---- reference :73-83
    def _unetr_forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.device)
        encoder = self.unetr.encoder
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in encoder.parameters())):
            return self.unetr(x)                                       # a frozen encoder: the inference kernels, no tape
        # the encoder trains: ``UNETR.forward`` with the encoder on the differentiable HIP primitives (``SamTrainer``'s own path)
        import torch.nn.functional as F
        from ..models.unetr import IMG_SIZE
        from .encoders import image_encoder_forward
        original = tuple(x.shape[-2:])
        scale = IMG_SIZE / max(original)
        size = (int(original[0] * scale + 0.5), int(original[1] * scale + 0.5))
        x = F.interpolate(x.float(), size, mode="bilinear", align_corners=False)
        x = (x - self.unetr.pixel_mean.to(x.device)) / self.unetr.pixel_std.to(x.device)
        x = F.pad(x, (0, IMG_SIZE - size[1], 0, IMG_SIZE - size[0]))
        z12 = encoder.forward_taped(x) if hasattr(encoder, "forward_taped") else image_encoder_forward(encoder, x)
        return self.unetr.postprocess_masks(self.unetr.decode(z12.float()), size, original)

    def _instance_iteration(self, x, y, metric_for_val: bool = False):
        outputs = self._unetr_forward(x)
        loss = self.instance_loss(outputs, y)
        if metric_for_val:
            return loss, self.instance_metric(outputs, y)
        return loss

    # ---- reference :85-131: two optimisation passes per iteration
    def train_iteration(self, x, y) -> dict:
        self.model.train()
        self.unetr.train()
        labels_instances, labels_for_unetr = self._split_targets(y)
        (loss, mask_loss, iou_loss, model_iou, _), reduced = self._optimization_pass(
            lambda: self._interactive_train_iteration(x, labels_instances))
        (unetr_loss,), reduced_unetr = self._optimization_pass(lambda: (self._instance_iteration(x, labels_for_unetr),))
        rec = {"iteration": self._iteration, "loss": float(loss.detach()), "mask_loss": float(mask_loss.detach()),
               "iou_regression_loss": float(iou_loss.detach()), "model_iou": float(model_iou), "instance_loss": float(unetr_loss.detach()),
               "allreduce_bytes": reduced + reduced_unetr}
        self.history.append(rec)
        self._iteration += 1
        return rec

    # ---- reference :133-180
    @torch.no_grad()
    def validate(self, loader: Iterable) -> float:
        """The reference's validation metric: per batch the interactive metric (the dice loss of the masks) + the decoder's metric / 3,
        averaged over the loader."""
        self.model.eval()
        self.unetr.eval()
        total, n = 0.0, 0
        for i, (x, y) in enumerate(loader):
            labels_instances, labels_for_unetr = self._split_targets(y)
            *_, metric = self._interactive_val_iteration(x, labels_instances, i)
            _, unetr_metric = self._instance_iteration(x, labels_for_unetr, metric_for_val=True)
            total += float(metric) + float(unetr_metric) / 3
            n += 1
        if n == 0:
            raise ValueError("JointSamTrainer.validate: the loader is empty")
        return total / n

    # ---- reference :39-71
    def save_checkpoint(self, path: str, **extra_save_dict) -> None:
        """``model_state`` (the ``TrainableSAM``: keys ``sam.*``), ``decoder_state`` (the UNETR's keys that do not start with ``encoder``),
        the optimizer's state and the iteration - plain tensors and numbers, so that the file loads with ``weights_only=True``."""
        decoder_state = OrderedDict((k, v.detach().cpu()) for k, v in self.unetr.state_dict().items() if not k.startswith("encoder"))
        model_state = OrderedDict((k, v.detach().cpu()) for k, v in self.model.state_dict().items())
        torch.save({"model_state": model_state, "decoder_state": decoder_state, "optimizer_state": self.optimizer.state_dict(),
                    "iteration": self._iteration, **extra_save_dict}, path)

    def load_checkpoint(self, path: str) -> dict:
        save_dict = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(save_dict["model_state"])
        self.optimizer.load_state_dict(save_dict["optimizer_state"])
        self._iteration = int(save_dict["iteration"])
        prune_prefix = "sam.image_"                                    # sam.image_encoder.* -> encoder.*
        encoder_state = [(k[len(prune_prefix):], v) for k, v in save_dict["model_state"].items() if k.startswith(prune_prefix)]
        self.unetr.load_state_dict(OrderedDict(encoder_state + list(save_dict["decoder_state"].items())))
        return save_dict
