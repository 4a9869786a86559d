"""The simple volumetric semantic SAM (reference ``micro_sam/models/simple_sam_3d_wrapper.py``): ``get_simple_sam_3d_model``,
``SimpleSam3DWrapper``, ``BasicBlock`` and ``SegmentationHead`` with the reference's names, signatures and ``state_dict`` keys
(``sam.*``, ``decoders.{0..3}.{conv1,conv2,downsample}.0.{weight,bias}``, ``out_conv.conv_pred.0.*``,
``out_conv.segmentation_head.*``; the normalisations, activations and up-samplings have no parameters and no key).

The SAM image encoder runs per slice; a convolutional decoder trained from scratch turns the [256, D, 64, 64] features into logits of
any number of classes: four blocks 256 -> 128 -> 64 -> 32 -> 16, each
    up_{(1, 2, 2)}(leaky_relu(IN(conv_3(leaky_relu(IN(conv_3(x))))) + IN(conv_1(x))))       (IN = InstanceNorm3d, no affine)
and a head conv_3 (16 -> 8), IN, leaky_relu, conv_1 (8 -> classes).

Everything between the encoder and the logits runs CHANNELS-LAST, [B, D, H, W, C]: the 3 x 3 x 3 convolutions by
``training.functional.conv3d_k3`` (csrc/conv3d.hip: an implicit-GEMM MFMA kernel with K = 27 Ci, no im2col copy, no padded copy, no
permute to channels-first), the normalisations fused with the residual sum and the activation by ``functional.instance_norm_act``, the
1 x 1 x 1 convolutions by ``functional.linear``.  The nearest up-sampling is a torch expand.  The ``nn.Conv3d`` modules only HOLD the
parameters (torch's default initialisation, checkpoints interchange with the reference); their ``forward`` is never called.

The encoder: frozen and without LoRA it is evaluated by the inference kernels under ``torch.no_grad()``, in batches of slices;
otherwise by the taped composition ``training.encoders.image_encoder_forward``.

Differences from the reference: slices smaller than 1024 x 1024 are normalised and zero-padded by ``Sam.preprocess`` (as ``Sam3DWrapper``
does) and the logits are cropped back to the slice size, so that ``SemanticSamTrainer`` can feed it the records it feeds the other
models; a 1024 x 1024 slice goes through normalisation alone.
Limits of this build: 1024 x 1024 token geometry (``build_sam``), vit_b / vit_l / vit_h.
PARITY: the convolution is pinned against torch's ``Conv3d`` (tests/conv3d_ref.py), the normalisation against fp64
``instance_norm`` (tests/instnorm_ref.py) and the decoder against its fp64 restatement (tests/test_gpu_simple_sam3d.py); the reference's
wrapper itself could not be run (``segment_anything`` is not installed)."""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Union

import torch
from torch import nn

from ..modeling import GRID, IMG_SIZE, PROMPT_DIM
from ..training import functional as HF

_VIT = ("vit_b", "vit_l", "vit_h")
SLICE_BATCH = 4                          # slices per call of the frozen encoder


def get_simple_sam_3d_model(device: Union[str, torch.device], n_classes: int, image_size: int, lora_rank: Optional[int] = None,
                            freeze_encoder: bool = False, model_type: str = "vit_b",
                            checkpoint_path: Optional[Union[str, os.PathLike]] = None,
                            state_dict: Optional[Dict[str, torch.Tensor]] = None) -> "SimpleSam3DWrapper":
    """Reference ``get_simple_sam_3d_model``: a SAM (optionally after LoRA surgery of rank ``lora_rank``) loaded flexibly from the
    checkpoint, with a convolutional decoder for ``n_classes`` classes (any number).  ``state_dict`` (extension, as
    ``util.get_sam_model``): upstream-named weights instead of a file."""
    from .. import util
    if model_type[:5] not in _VIT:
        raise ValueError(f"'{model_type}' is not a supported choice of model.")
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 1:
        raise ValueError(f"get_simple_sam_3d_model: n_classes must be a positive int, got {n_classes!r}")
    if image_size != IMG_SIZE:
        raise NotImplementedError(f"micro_sam_amd: get_simple_sam_3d_model supports image_size == {IMG_SIZE} only (build_sam builds the "
                                  f"{GRID} x {GRID} token grid), got {image_size}")
    peft_kwargs = {}
    if lora_rank is not None:
        from .peft_sam import LoRASurgery
        peft_kwargs = {"rank": lora_rank, "peft_module": LoRASurgery}
    _, sam = util.get_sam_model(model_type=model_type, device=device, checkpoint_path=checkpoint_path, return_sam=True,
                                flexible_load_checkpoint=True, peft_kwargs=peft_kwargs, state_dict=state_dict)
    # LoRA trains the encoder's low-rank matrices: never freeze it then
    sam_3d = SimpleSam3DWrapper(sam, num_classes=n_classes, freeze_encoder=freeze_encoder if lora_rank is None else False)
    sam_3d.to(device)
    return sam_3d


def _conv(ci: int, co: int, k: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv3d(ci, co, kernel_size=k, stride=1, padding=k // 2, bias=True))


def _pointwise(x: torch.Tensor, conv: nn.Conv3d) -> torch.Tensor:
    """A 1 x 1 x 1 convolution of a channels-last volume: one linear map per voxel."""
    return HF.linear(x, conv.weight.reshape(conv.weight.shape[0], conv.weight.shape[1]), conv.bias)


def upsample_hw(x: torch.Tensor) -> torch.Tensor:
    """``nn.Upsample(scale_factor=(1, 2, 2), mode="nearest")`` of a channels-last volume [B, D, H, W, C]."""
    B, D, H, W, C = x.shape
    return x[:, :, :, None, :, None, :].expand(B, D, H, 2, W, 2, C).reshape(B, D, 2 * H, 2 * W, C)


class BasicBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv1 = _conv(in_channels, out_channels, 3)
        self.conv2 = _conv(out_channels, out_channels, 3)
        self.downsample = _conv(in_channels, out_channels, 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, D, H, W, in_channels] -> [B, D, 2 H, 2 W, out_channels] (channels-last)."""
        c1, c2 = self.conv1[0], self.conv2[0]
        residual = _pointwise(x, self.downsample[0])
        out = HF.instance_norm_act(HF.conv3d_k3(x, c1.weight, c1.bias))
        out = HF.instance_norm_act(HF.conv3d_k3(out, c2.weight, c2.bias), residual=residual)
        return upsample_hw(out)


class SegmentationHead(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv_pred = _conv(in_channels, in_channels // 2, 3)
        self.segmentation_head = nn.Conv3d(in_channels // 2, out_channels, kernel_size=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, D, H, W, in_channels] -> logits [B, D, H, W, out_channels] (channels-last)."""
        c = self.conv_pred[0]
        return _pointwise(HF.instance_norm_act(HF.conv3d_k3(x, c.weight, c.bias)), self.segmentation_head)


class SimpleSam3DWrapper(nn.Module):
    def __init__(self, sam, num_classes: int, freeze_encoder: bool):
        """``sam``: the ``modeling.Sam`` whose image encoder is used; ``num_classes``: output channels of the decoder;
        ``freeze_encoder``: no gradients for the image encoder, which then runs the inference kernels."""
        super().__init__()
        if hasattr(sam.image_encoder, "forward_taped"):                        # TinyViT
            raise ValueError("'vit_t' is not a supported choice of model.")
        self.sam = sam
        self.freeze_encoder = freeze_encoder
        if self.freeze_encoder:
            for param in self.sam.image_encoder.parameters():
                param.requires_grad = False
        self.decoders = nn.ModuleList([BasicBlock(256, 128), BasicBlock(128, 64), BasicBlock(64, 32), BasicBlock(32, 16)])
        self.out_conv = SegmentationHead(16, num_classes)

    def _apply_image_encoder(self, slices: torch.Tensor) -> torch.Tensor:
        """[N, 3, 1024, 1024] normalised + padded slices -> [N, 256, 64, 64]."""
        enc = self.sam.image_encoder
        if self.freeze_encoder:
            with torch.no_grad():
                return torch.cat([enc(part) for part in slices.split(SLICE_BATCH)], dim=0).float()
        from ..training.encoders import image_encoder_forward
        return image_encoder_forward(enc, slices)

    def decode(self, features: torch.Tensor) -> torch.Tensor:
        """Encoder features [B, D, 64, 64, 256] (channels-last) -> logits [B, D, 1024, 1024, classes]."""
        out = features
        for decoder in self.decoders:
            out = decoder(out)
        return self.out_conv(out)

    def forward(self, batched_input: List[Dict[str, Any]], multimask_output: bool) -> List[Dict[str, torch.Tensor]]:
        """Automatic (prompt-free) segmentation of volumes.  Every record: 'image' float [3, D, H, W] with H, W <= 1024, the same shape
        for all records.  -> per volume 'masks' [1, classes, D, H, W] (logits).  ``multimask_output`` is accepted for the trainer's
        sake; the decoder has one output per class."""
        sam = self.sam
        images = torch.stack([rec["image"] for rec in batched_input], dim=0).to(sam.device).float()
        if images.dim() != 5 or images.shape[1] != 3 or max(images.shape[-2:]) > IMG_SIZE:
            raise ValueError(f"SimpleSam3DWrapper: every image must be [3, D, H, W] with H, W <= {IMG_SIZE}, got a batch of shape "
                             f"{tuple(images.shape)}")
        batch, depth, height, width = int(images.shape[0]), int(images.shape[2]), int(images.shape[3]), int(images.shape[4])
        slices = images.transpose(1, 2).reshape(batch * depth, 3, height, width)
        features = self._apply_image_encoder(sam.preprocess(slices))
        features = features.permute(0, 2, 3, 1).reshape(batch, depth, GRID, GRID, PROMPT_DIM)
        logits = self.decode(features)[:, :, :height, :width, :].permute(0, 4, 1, 2, 3)
        return [{"masks": m.unsqueeze(0)} for m in logits]
