"""PEFT surgery of the image encoder (reference ``micro_sam/models/peft_sam.py``).

``PEFT_Sam(sam, rank, peft_module=LoRASurgery, ...)`` replaces ``block.attn.qkv`` (and ``block.mlp`` with
``update_matrices=[..., "mlp"]``) by modules with the reference's names and parameters (``qkv_proj``, ``w_a_linear_q``,
``w_b_linear_q``, ...), so LoRA checkpoints of micro_sam ``load_state_dict`` unchanged.  At inference a low-rank update is
a weight update - ``qkv(x) + B A x == (W + B A) x`` - so the HIP encoder needs no extra kernel: the modules expose the MERGED
``weight`` / ``bias`` that ``ImageEncoderViT._prepare`` turns into its 16-bit operand copies (exact; alpha = 1 as in the
reference).  Training keeps the low-rank branches as separate products so that A and B receive gradients
(``training/encoders.py`` ``_qkv_projection`` / ``_mlp``: the frozen projection plus ``alpha * B(A(x))``; first GPU run
pending, composition checked on the CPU in tests/test_training_encoders_host.py).  The reference's other methods follow the same
plan with the reference's module and parameter names: FacT (``FacTSurgery``: a rank-r update of the q and v rows) and SSF
(``ScaleShiftLayer``: a per-channel affine map folded into each linear's weight and bias and each LayerNorm's gamma and beta) are
weight updates read through the same merged ``weight`` / ``bias``; the selective surgeries (``AttentionSurgery``, ``BiasSurgery``,
``LayerNormSurgery``, ``ClassicalSurgery``) only set ``requires_grad``; ``AdaptFormer`` adds a non-linear branch next to the MLP that
no re-parameterisation removes - the 16-bit encoder runs it as one fused launch (``csrc/adapter.hip``, ``msam_adapter_bf16``), the
strict modes compose it from their fp32 products, the fp8 mode refuses it.  QLoRA (``quantize=True``) is not provided.
"""
from __future__ import annotations

import math
from typing import List, Optional, Union

import torch
import torch.nn as nn


class AttentionLoRA(nn.Module):
    def __init__(self, rank: int, block: nn.Linear, update_matrices: List[str] = ["q", "v"]):
        super().__init__()
        self.qkv_proj = block
        self.dim = self.qkv_proj.in_features
        self.alpha = 1
        self.rank = rank
        for m in ("q", "v", "k"):
            if m in update_matrices:
                setattr(self, f"w_a_linear_{m}", nn.Linear(self.dim, rank, bias=False))
                setattr(self, f"w_b_linear_{m}", nn.Linear(rank, self.dim, bias=False))
        self.reset_parameters()

    def reset_parameters(self):
        for m in ("q", "v", "k"):
            if hasattr(self, f"w_a_linear_{m}"):
                nn.init.kaiming_uniform_(getattr(self, f"w_a_linear_{m}").weight, a=math.sqrt(5))
                nn.init.zeros_(getattr(self, f"w_b_linear_{m}").weight)

    @property
    def in_features(self) -> int:
        return self.qkv_proj.in_features

    @property
    def out_features(self) -> int:
        return self.qkv_proj.out_features

    @property
    def weight(self) -> torch.Tensor:
        """[3 dim, dim] with the low-rank updates merged into the q / k / v row blocks."""
        w = self.qkv_proj.weight.detach().clone()
        for m, sl in (("q", slice(0, self.dim)), ("k", slice(self.dim, 2 * self.dim)), ("v", slice(2 * self.dim, 3 * self.dim))):
            if hasattr(self, f"w_a_linear_{m}"):
                w[sl] += self.alpha * (getattr(self, f"w_b_linear_{m}").weight.detach() @ getattr(self, f"w_a_linear_{m}").weight.detach())
        return w

    @property
    def bias(self) -> torch.Tensor:
        return self.qkv_proj.bias


class _MergedLinear:
    """``lin1`` / ``lin2`` of an ``MLPLoRA`` as the encoder reads them: merged weight, original bias."""

    def __init__(self, lin: nn.Linear, a: nn.Linear, b: nn.Linear):
        self._lin, self._a, self._b = lin, a, b

    @property
    def weight(self) -> torch.Tensor:
        return self._lin.weight.detach() + self._b.weight.detach() @ self._a.weight.detach()

    @property
    def bias(self) -> torch.Tensor:
        return self._lin.bias

    @property
    def in_features(self) -> int:
        return self._lin.in_features

    @property
    def out_features(self) -> int:
        return self._lin.out_features


class MLPLoRA(nn.Module):
    def __init__(self, rank: int, mlp_layer: nn.Module):
        super().__init__()
        self.mlp_layer = mlp_layer
        self.rank = rank
        self.w_a_linear_1 = nn.Linear(mlp_layer.lin1.in_features, rank, bias=False)
        self.w_b_linear_1 = nn.Linear(rank, mlp_layer.lin1.out_features, bias=False)
        self.w_a_linear_2 = nn.Linear(mlp_layer.lin2.in_features, rank, bias=False)
        self.w_b_linear_2 = nn.Linear(rank, mlp_layer.lin2.out_features, bias=False)
        self.activation = mlp_layer.act
        nn.init.kaiming_uniform_(self.w_a_linear_1.weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.w_a_linear_2.weight, a=math.sqrt(5))
        nn.init.zeros_(self.w_b_linear_1.weight)
        nn.init.zeros_(self.w_b_linear_2.weight)

    @property
    def lin1(self):
        return _MergedLinear(self.mlp_layer.lin1, self.w_a_linear_1, self.w_b_linear_1)

    @property
    def lin2(self):
        return _MergedLinear(self.mlp_layer.lin2, self.w_a_linear_2, self.w_b_linear_2)

    @property
    def act(self):
        return self.activation


class LoRASurgery(nn.Module):
    def __init__(self, rank: int, block: nn.Module, update_matrices: List[str] = ["q", "v"]):
        super().__init__()
        if set(update_matrices) - set(["q", "k", "v", "mlp"]):
            raise ValueError(f"Some of the expected keys for updating matrics in '{update_matrices}' are not expected.")
        self.block = block
        block.attn.qkv = AttentionLoRA(rank=rank, block=block.attn.qkv, update_matrices=update_matrices)
        if "mlp" in update_matrices:
            block.mlp = MLPLoRA(rank=rank, mlp_layer=block.mlp)

    def forward(self, x):
        return x


class FacTSurgery(nn.Module):
    """Factor tuning of the attention projection: the module takes the place of ``block.attn.qkv``; ``FacTu`` [r, D] and ``FacTv``
    [D, r] are the shared factors, ``q_FacTs`` / ``v_FacTs`` [r, r] the cores of the q and the v update.  Inference reads the merged
    ``weight``: ``W_q += FacTv q_FacTs FacTu`` on rows [0, D), ``W_v += FacTv v_FacTs FacTu`` on rows [2 D, 3 D), formed in fp32; the
    dropout between core and ``FacTv`` acts in training only (training/encoders.py)."""

    def __init__(self, rank: int, block: nn.Module, dropout: Optional[float] = 0.1):
        super().__init__()
        self.qkv_proj = block.attn.qkv
        self.dim = self.qkv_proj.in_features
        self.q_FacTs = nn.Linear(rank, rank, bias=False)
        self.v_FacTs = nn.Linear(rank, rank, bias=False)
        self.dropout = dropout
        if self.dropout is not None:
            self.dp_q = nn.Dropout(self.dropout)
            self.dp_v = nn.Dropout(self.dropout)
        self.FacTu = nn.Linear(self.dim, rank, bias=False)
        self.FacTv = nn.Linear(rank, self.dim, bias=False)
        block.attn.qkv = self

    @property
    def in_features(self) -> int:
        return self.qkv_proj.in_features

    @property
    def out_features(self) -> int:
        return self.qkv_proj.out_features

    @property
    def weight(self) -> torch.Tensor:
        """[3 dim, dim] with the factorised updates merged into the q and v row blocks (fp32)."""
        w = self.qkv_proj.weight.detach().to(torch.float32).clone()
        u, v = self.FacTu.weight.detach().to(torch.float32), self.FacTv.weight.detach().to(torch.float32)
        w[:self.dim] += v @ self.q_FacTs.weight.detach().to(torch.float32) @ u
        w[2 * self.dim:] += v @ self.v_FacTs.weight.detach().to(torch.float32) @ u
        return w

    @property
    def bias(self) -> torch.Tensor:
        return self.qkv_proj.bias


class ScaleShiftLayer(nn.Module):
    """SSF: ``layer(x) * scale + shift`` per output channel around a linear layer or a LayerNorm.  Inference reads the map folded into
    the layer's own parameters (fp32): a linear's ``W' = scale[:, None] W``, ``b' = scale b + shift``; a LayerNorm's
    ``gamma' = scale gamma``, ``beta' = scale beta + shift``."""

    def __init__(self, layer: nn.Module, dim: int):
        super().__init__()
        self.layer = layer
        self.scale = nn.Parameter(torch.normal(mean=1.0, std=0.2, size=(dim,)))
        self.shift = nn.Parameter(torch.normal(mean=0.0, std=0.2, size=(dim,)))

    @property
    def weight(self) -> torch.Tensor:
        w = self.layer.weight.detach().to(torch.float32)
        s = self.scale.detach().to(torch.float32)
        return s.reshape(-1, *([1] * (w.dim() - 1))) * w

    @property
    def bias(self) -> torch.Tensor:
        s, t = self.scale.detach().to(torch.float32), self.shift.detach().to(torch.float32)
        b = self.layer.bias
        return t.clone() if b is None else s * b.detach().to(torch.float32) + t

    @property
    def in_features(self) -> int:
        return self.layer.in_features

    @property
    def out_features(self) -> int:
        return self.layer.out_features

    @property
    def eps(self) -> float:
        return self.layer.eps

    @property
    def normalized_shape(self):
        return self.layer.normalized_shape


class SSFSurgery(nn.Module):
    """Scale-and-shift layers around the four linear layers and the two LayerNorms of a block (``rank`` is unused, as in the reference)."""

    def __init__(self, rank: Optional[int], block: nn.Module):
        super().__init__()
        self.block = block
        if hasattr(block, "attn"):
            block.attn.qkv = ScaleShiftLayer(block.attn.qkv, block.attn.qkv.in_features * 3)
            block.attn.proj = ScaleShiftLayer(block.attn.proj, block.attn.proj.in_features)
            block.mlp.lin1 = ScaleShiftLayer(block.mlp.lin1, block.mlp.lin1.out_features)
            block.mlp.lin2 = ScaleShiftLayer(block.mlp.lin2, block.mlp.lin2.out_features)
            block.norm1 = ScaleShiftLayer(block.norm1, block.norm1.normalized_shape[0])
            block.norm2 = ScaleShiftLayer(block.norm2, block.norm2.normalized_shape[0])
        # Any other module is left as it is.  That includes the patch embedding, which the reference hands over as well: its second
        # branch asks for an attribute ``patch_embed`` of the patch embedding itself, which does not exist, so a reference SSF checkpoint
        # carries no scale / shift there - and none is added here.

    def forward(self, x):
        return x


class SelectiveSurgery(nn.Module):
    """Base of the surgeries that add nothing and only choose which of a block's parameters train."""

    def __init__(self, block: nn.Module):
        super().__init__()
        self.block = block

    def allow_gradient_update_for_parameters(self, prefix: Optional[List[str]] = None, suffix: Optional[List[str]] = None,
                                             infix: Optional[List[str]] = None):
        for name, param in self.block.named_parameters():
            if ((prefix is not None and name.startswith(tuple(prefix))) or (suffix is not None and name.endswith(tuple(suffix))) or
                    (infix is not None and any(part in name for part in infix))):
                param.requires_grad = True

    def forward(self, x):
        return x


class AttentionSurgery(SelectiveSurgery):
    def __init__(self, block: nn.Module):
        super().__init__(block=block)
        self.allow_gradient_update_for_parameters(prefix=["attn"])


class BiasSurgery(SelectiveSurgery):
    def __init__(self, block: nn.Module):
        super().__init__(block=block)
        self.allow_gradient_update_for_parameters(suffix=["bias"])


class LayerNormSurgery(SelectiveSurgery):
    def __init__(self, block: nn.Module):
        super().__init__(block=block)
        self.allow_gradient_update_for_parameters(infix=["norm1", "norm2"])


class ClassicalSurgery(SelectiveSurgery):
    """Plain fine-tuning of the chosen blocks: every parameter of the block trains."""

    def __init__(self, block: nn.Module):
        super().__init__(block=block)
        for param in self.block.parameters():
            param.requires_grad = True


class AdaptFormer(nn.Module):
    """The module takes the place of ``block.mlp``: ``y + mlp_proj(y) + alpha * up_proj(relu(down_proj(y)))`` for the block's
    ``y = norm2(x)`` - the adapter's own residual is its INPUT, the normed stream, on top of the block's residual ``x`` (the
    reference's behaviour, which trained checkpoints expect).  ``alpha``: ``"learnable_scalar"`` (a parameter [1], initially 1) or a
    fixed number; ``rank`` is unused.  ``lin1`` / ``lin2`` / ``act`` are those of the wrapped MLP, which is how the encoders read it;
    the branch itself is ``msam_adapter_bf16`` at inference (``ImageEncoderViT._prepare``)."""

    def __init__(self, rank: Optional[int], block: nn.Module, alpha: Optional[Union[str, float]] = "learnable_scalar",
                 dropout: Optional[float] = None, projection_size: int = 64):
        super().__init__()
        self.mlp_proj = block.mlp
        self.n_embd = block.mlp.lin1.in_features
        if isinstance(alpha, str):
            if alpha != "learnable_scalar":
                raise ValueError(f"AdaptFormer: alpha must be 'learnable_scalar' or a number, got {alpha!r}")
            self.alpha = nn.Parameter(torch.ones(1))
        else:
            self.alpha = alpha
        self.projection_size = projection_size
        self.dropout = dropout
        self.down_proj = nn.Linear(self.n_embd, self.projection_size)
        self.non_linear_func = nn.ReLU()
        self.up_proj = nn.Linear(self.projection_size, self.n_embd)
        block.mlp = self
        if self.dropout is not None:
            self.dropout_layer = nn.Dropout(self.dropout)
        nn.init.kaiming_uniform_(self.down_proj.weight, a=math.sqrt(5))
        nn.init.zeros_(self.up_proj.weight)
        nn.init.zeros_(self.down_proj.bias)
        nn.init.zeros_(self.up_proj.bias)

    @property
    def lin1(self):
        return self.mlp_proj.lin1

    @property
    def lin2(self):
        return self.mlp_proj.lin2

    @property
    def act(self):
        return self.mlp_proj.act


_RANKED = (LoRASurgery, FacTSurgery)
_SUPPORTED = _RANKED + (SelectiveSurgery, SSFSurgery, AdaptFormer)


class PEFT_Sam(nn.Module):
    """Reference ``PEFT_Sam``: the surgery ``peft_module`` applied to the chosen blocks of the image encoder, whose other parameters
    are frozen first; ``.sam`` is the operated model."""

    def __init__(self, model, rank: Optional[int] = None, peft_module=LoRASurgery,
                 attention_layers_to_update: Optional[List[int]] = None, quantize: bool = False, **module_kwargs):
        super().__init__()
        if not (isinstance(peft_module, type) and issubclass(peft_module, _SUPPORTED)):
            raise NotImplementedError(f"micro_sam_amd: {peft_module!r} is not a PEFT surgery (LoRASurgery, FacTSurgery, SSFSurgery, "
                                      "AdaptFormer, AttentionSurgery, BiasSurgery, LayerNormSurgery, ClassicalSurgery)")
        if quantize:
            raise NotImplementedError("micro_sam_amd: QLoRA (bitsandbytes 4-bit) is not provided")
        if issubclass(peft_module, _RANKED) and (not rank or rank <= 0):
            raise RuntimeError("The chosen PEFT method cannot run without a valid rank choice.")
        blocks = model.image_encoder.blocks
        if attention_layers_to_update and set(attention_layers_to_update) - set(range(len(blocks))):
            raise ValueError("The chosen layer(s) to apply PEFT method is not a valid transformer block id.")
        self.peft_layers = attention_layers_to_update or list(range(len(blocks)))
        self.peft_module = peft_module
        self.peft_blocks = []
        for param in model.image_encoder.parameters():
            param.requires_grad = False
        if issubclass(peft_module, SSFSurgery):
            self.peft_blocks.append(peft_module(rank=rank, block=model.image_encoder.patch_embed))      # adds nothing (SSFSurgery)
        for t_layer_i, blk in enumerate(blocks):
            if t_layer_i not in self.peft_layers:
                continue
            if issubclass(peft_module, SelectiveSurgery):
                self.peft_blocks.append(peft_module(block=blk))
            else:
                self.peft_blocks.append(peft_module(rank=rank, block=blk, **module_kwargs))
        self.peft_blocks = nn.ModuleList(self.peft_blocks)
        self.sam = model
        model.image_encoder.invalidate()

    def forward(self, batched_input, multimask_output):
        raise NotImplementedError("micro_sam_amd: use the SamPredictor / TrainableSAM interfaces")
