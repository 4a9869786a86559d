"""The volumetric semantic SAM (reference ``micro_sam/models/sam_3d_wrapper.py``): ``get_sam_3d_model``, ``Sam3DWrapper``,
``ImageEncoderViT3DWrapper`` and ``NDBlockWrapper`` with the reference's names, signatures and ``state_dict`` keys
(``sam_model.image_encoder.image_encoder.blocks.{i}.block.*``, ``...blocks.{i}.adapter_linear_down.weight``,
``...adapter_conv.weight`` [384, 384, 3, 1, 1], ``...adapter_norm_2.*`` and so on).

The model treats the D slices of a volume as a batch of images; what makes it 3-d are two adapters per transformer block (before the
attention and before the MLP) that mix every token with the same token of the neighbouring slices:
    x + up(gelu(conv_{3 x 1 x 1}(down(LayerNorm(x)))))
with 384 adapter channels.  The depth convolution runs on token-major rows by ``training.functional.depth_conv3`` (csrc/conv3d.hip: an
implicit-shift MFMA GEMM, no im2col copy and no permute to channels-first); the two projections are ``functional.linear``.

The forward pass is ONE taped composition in the style of ``training.encoders.image_encoder_forward`` - under autograd for training,
under ``torch.no_grad()`` for evaluation.  It never calls ``modeling.ImageEncoderViT.forward``: the inference kernels behind that walk
the un-wrapped blocks.  The decoder takes all B D embeddings in one ``mask_decoder_forward`` call (no prompts: an empty sparse
embedding and ``no_mask_embed`` as the dense one, the reference's broadcast written out).

Limits of this build: three classes (``modeling.MaskDecoder`` has three multi-mask outputs) and 1024 x 1024 slices (``build_sam``);
``models.simple_sam_3d_wrapper.SimpleSam3DWrapper`` (a per-slice encoder with a 3 x 3 x 3 convolutional decoder) takes any number of classes.
PARITY: the depth convolution is pinned against torch's ``Conv3d`` (tests/depth_conv_ref.py) and the block against its fp64 restatement
(tests/test_gpu_sam3d.py); the reference's wrapper itself could not be run (``segment_anything`` is not installed)."""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Type, Union

import torch
import torch.nn.functional as F
from torch import nn

from ..modeling import GRID, IMG_SIZE, PATCH, PROMPT_DIM
from ..training import functional as HF
from ..training.encoders import _attention, _mlp, _norm, _window_partition, _window_unpartition

_VIT = {"vit_b": (768, 12), "vit_l": (1024, 16), "vit_h": (1280, 16)}


def get_sam_3d_model(device: Union[str, torch.device], n_classes: int, image_size: int, lora_rank: Optional[int] = None,
                     freeze_encoder: bool = False, model_type: str = "vit_b",
                     checkpoint_path: Optional[Union[str, os.PathLike]] = None,
                     state_dict: Optional[Dict[str, torch.Tensor]] = None) -> "Sam3DWrapper":
    """Reference ``get_sam_3d_model``: a SAM (optionally after LoRA surgery of rank ``lora_rank``) loaded flexibly from the checkpoint
    and wrapped for volumes.  ``state_dict`` (extension, as ``util.get_sam_model``): upstream-named weights instead of a file."""
    from ..util import get_sam_model
    if model_type[:5] not in _VIT:
        raise ValueError(f"'{model_type}' is not a supported choice of model.")
    if n_classes != 3:
        raise NotImplementedError(f"micro_sam_amd: get_sam_3d_model supports n_classes == 3 only (modeling.MaskDecoder has three "
                                  f"multi-mask outputs), got {n_classes}")
    if image_size != IMG_SIZE:
        raise NotImplementedError(f"micro_sam_amd: get_sam_3d_model supports image_size == {IMG_SIZE} only (build_sam builds the "
                                  f"{GRID} x {GRID} token grid), got {image_size}")
    peft_kwargs = {}
    if lora_rank is not None:
        from .peft_sam import LoRASurgery
        peft_kwargs = {"rank": lora_rank, "peft_module": LoRASurgery}
    _, sam = get_sam_model(model_type=model_type, device=device, checkpoint_path=checkpoint_path, return_sam=True,
                           flexible_load_checkpoint=True, peft_kwargs=peft_kwargs, state_dict=state_dict)
    # LoRA trains the encoder's low-rank matrices: never freeze it then
    sam_3d = Sam3DWrapper(sam, freeze_encoder=freeze_encoder if lora_rank is None else False, model_type=model_type[:5])
    sam_3d.to(device)
    return sam_3d


class Sam3DWrapper(nn.Module):
    def __init__(self, sam_model, freeze_encoder: bool, model_type: str = "vit_b"):
        """``sam_model``: the ``modeling.Sam`` to wrap (its image encoder is replaced by the 3-d one); ``freeze_encoder``: no gradients
        for the image encoder, adapters included; ``model_type``: vit_b, vit_l or vit_h."""
        super().__init__()
        if model_type not in _VIT:
            raise ValueError(f"'{model_type}' is not a supported choice of model.")
        embed_dim, num_heads = _VIT[model_type]
        enc = sam_model.image_encoder
        # an encoder of another size (the tests' two-block one) says what it is
        embed_dim, num_heads = getattr(enc, "embed_dim", embed_dim), getattr(enc, "num_heads", num_heads)
        sam_model.image_encoder = ImageEncoderViT3DWrapper(image_encoder=enc, num_heads=num_heads, embed_dim=embed_dim)
        self.sam_model = sam_model
        self.freeze_encoder = freeze_encoder
        if self.freeze_encoder:
            for param in self.sam_model.image_encoder.parameters():
                param.requires_grad = False

    def forward(self, batched_input: List[Dict[str, Any]], multimask_output: bool) -> List[Dict[str, torch.Tensor]]:
        """Automatic (prompt-free) segmentation of volumes.  Every record: 'image' float [3, D, H, W] with H = W <= 1024, already resized
        for the model, and 'original_size' (H, W), the same for all records.  -> per volume 'masks' [1, C, D, H, W] (logits at the
        original size), 'iou_predictions' [D, C] and 'low_res_logits' [1, C, D, 256, 256]; C = 3 with ``multimask_output``."""
        from ..training.trainable_sam import mask_decoder_forward, postprocess_masks
        sam = self.sam_model
        images = torch.stack([rec["image"] for rec in batched_input], dim=0).to(sam.device).float()
        original_size = batched_input[0]["original_size"]
        if any(tuple(rec["original_size"]) != tuple(original_size) for rec in batched_input):
            raise ValueError("Sam3DWrapper: all volumes of a batch must share one original_size")
        if images.dim() != 5 or images.shape[1] != 3 or images.shape[-1] != images.shape[-2]:
            raise ValueError(f"Sam3DWrapper: every image must be [3, D, S, S], got a batch of shape {tuple(images.shape)}")
        batch, depth, side = int(images.shape[0]), int(images.shape[2]), int(images.shape[-1])
        # depth next to the batch: the transformer sees B D images
        slices = images.transpose(1, 2).reshape(batch * depth, 3, side, side)
        embeddings = sam.image_encoder(sam.preprocess(slices), depth)
        n = batch * depth
        sparse = torch.empty((n, 0, PROMPT_DIM), dtype=torch.float32, device=embeddings.device)
        dense = sam.prompt_encoder.no_mask_embed.weight.reshape(1, -1, 1, 1).expand(n, -1, GRID, GRID)
        low_res, iou = mask_decoder_forward(sam.mask_decoder, embeddings, sam.prompt_encoder.get_dense_pe(), sparse, dense,
                                            multimask_output)
        masks = postprocess_masks(low_res, (side, side), original_size)
        c = masks.shape[1]
        masks = masks.reshape(batch, depth, c, *masks.shape[-2:]).transpose(1, 2)
        low_res = low_res.reshape(batch, depth, c, *low_res.shape[-2:]).transpose(1, 2)
        iou = iou.reshape(batch, depth, c)
        return [{"masks": m.unsqueeze(0), "iou_predictions": i, "low_res_logits": l.unsqueeze(0)} for m, i, l in zip(masks, iou, low_res)]


class ImageEncoderViT3DWrapper(nn.Module):
    def __init__(self, image_encoder: nn.Module, num_heads: int = 12, embed_dim: int = 768, adapter_channels: int = 384):
        super().__init__()
        self.image_encoder = image_encoder
        self.img_size = self.image_encoder.img_size
        self.embed_dim = embed_dim
        for i, blk in enumerate(self.image_encoder.blocks):
            self.image_encoder.blocks[i] = NDBlockWrapper(block=blk, num_heads=num_heads, dim=embed_dim, adapter_channels=adapter_channels)

    def invalidate(self) -> None:
        """``modeling.Sam`` tells its encoder when parameters moved; nothing is cached here beyond what ``functional`` keys by version."""
        if hasattr(self.image_encoder, "invalidate"):
            self.image_encoder.invalidate()

    def forward(self, x: torch.Tensor, d_size: int) -> torch.Tensor:
        """[B D, 3, 1024, 1024] normalised + padded slices (the ``d_size`` slices of a volume consecutive) -> [B D, 256, 64, 64]."""
        enc = self.image_encoder
        n, width = x.shape[0], self.embed_dim
        if n % d_size != 0:
            raise ValueError(f"ImageEncoderViT3DWrapper: {n} slices are not volumes of {d_size}")
        # patch embedding: the 16 x 16 / 16 convolution as one linear map per patch, columns (c, ky, kx) like the weight
        patches = x.reshape(n, 3, GRID, PATCH, GRID, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(n, GRID, GRID, 3 * PATCH * PATCH)
        w = enc.patch_embed.proj.weight
        x = HF.linear(patches, w.reshape(w.shape[0], -1), enc.patch_embed.proj.bias)
        if enc.pos_embed is not None:
            x = x + enc.pos_embed
        for blk in enc.blocks:
            x = blk(x, d_size)
        conv1, ln1, conv3, ln2 = enc.neck[0], enc.neck[1], enc.neck[2], enc.neck[3]
        y = HF.linear(x, conv1.weight.reshape(PROMPT_DIM, width), None)                    # 1 x 1 convolution
        y = HF.layer_norm(y, ln1.weight, ln1.bias, ln1.eps)                                # LayerNorm2d = LayerNorm over the channels
        cols = F.unfold(y.permute(0, 3, 1, 2), kernel_size=3, padding=1).transpose(1, 2)   # [B D, 4096, 256 * 9], columns (c, ky, kx)
        y = HF.linear(cols, conv3.weight.reshape(PROMPT_DIM, -1), None).reshape(n, GRID, GRID, PROMPT_DIM)
        y = HF.layer_norm(y, ln2.weight, ln2.bias, ln2.eps)
        return y.permute(0, 3, 1, 2)


class NDBlockWrapper(nn.Module):
    def __init__(self, block: nn.Module, dim: int, num_heads: int, norm_layer: Type[nn.Module] = nn.LayerNorm,
                 adapter_channels: int = 384):
        super().__init__()
        self.block = block
        self.adapter_channels = adapter_channels
        for tag in ("", "_2"):
            setattr(self, "adapter_linear_down" + tag, nn.Linear(dim, adapter_channels, bias=False))
            setattr(self, "adapter_linear_up" + tag, nn.Linear(adapter_channels, dim, bias=False))
            setattr(self, "adapter_conv" + tag, nn.Conv3d(adapter_channels, adapter_channels, kernel_size=(3, 1, 1), padding="same"))
            setattr(self, "adapter_act" + tag, nn.GELU())
            setattr(self, "adapter_norm" + tag, norm_layer(dim))

    def _adapter(self, x: torch.Tensor, d_size: int, tag: str) -> torch.Tensor:
        norm, conv = getattr(self, "adapter_norm" + tag), getattr(self, "adapter_conv" + tag)
        y = HF.layer_norm(x, norm.weight, norm.bias, norm.eps)
        y = HF.linear(y, getattr(self, "adapter_linear_down" + tag).weight, None)
        y = HF.depth_conv3(y, conv.weight, conv.bias, d_size)                              # token-major: no permute to channels-first
        y = HF.linear(F.gelu(y), getattr(self, "adapter_linear_up" + tag).weight, None)
        return x + y

    def forward(self, x: torch.Tensor, d_size: int) -> torch.Tensor:
        """x [B D, 64, 64, dim] -> the same shape: adapter, attention, adapter, MLP, each with its residual."""
        blk = self.block
        x = self._adapter(x, d_size, "")
        y = _norm(blk.norm1, x)
        if blk.window_size > 0:
            hw = y.shape[1:3]
            y, pad_hw = _window_partition(y, blk.window_size)
            y = _window_unpartition(_attention(blk.attn, y), blk.window_size, pad_hw, hw)
        else:
            y = _attention(blk.attn, y)
        x = x + y
        x = self._adapter(x, d_size, "_2")
        y = _norm(blk.norm2, x)
        return x + _mlp(blk.mlp, y)
