"""``ops.semantic_loss`` and ``ops.semantic_loss_backward``: the Python side of csrc/semloss.hip (msam_semantic_loss_forward /
msam_semantic_loss_backward), the fused soft-max dice + cross-entropy loss of semantic-segmentation fine-tuning.  Defined here and
re-exported by micro_sam_amd/ops.py with the boundary checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); every
check runs before the first launch.  tests/test_semantic_loss_host.py and tests/test_gpu_semantic_loss.py run them."""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Tuple

import torch

from . import _lib

SEMLOSS_MAX_CLASSES = 32                                                # include/msam_hip.h MSAM_SEMLOSS_MAX_CLASSES
SEMLOSS_EPS = 1e-7                                                      # torch_em DiceLoss(eps=1e-7)

# per (device, stream): a byte workspace that only grows
_WS: Dict[Any, torch.Tensor] = {}


class SemanticLossStats(NamedTuple):
    """What the forward pass leaves for the backward pass and for the records, all on the device.  ``raw``: int64 [3 C + 5], the
    library's layout; the other fields are views of it: float64 ``num`` [C] = sum p_c t_c, ``psq`` [C] = sum p_c^2, ``ce_sum``, ``dice``
    and ``ce`` (0-dim: the two parts of the loss, unweighted), int64 ``count`` [C] = sum t_c, ``n_valid`` and ``n_ignored`` (0-dim)."""
    raw: torch.Tensor
    num: torch.Tensor
    psq: torch.Tensor
    ce_sum: torch.Tensor
    dice: torch.Tensor
    ce: torch.Tensor
    count: torch.Tensor
    n_valid: torch.Tensor
    n_ignored: torch.Tensor


def stats_views(raw: torch.Tensor, c: int) -> SemanticLossStats:
    f = raw.view(torch.float64)
    return SemanticLossStats(raw, f[:c], f[c:2 * c], f[2 * c], f[2 * c + 1], f[2 * c + 2], raw[2 * c + 3:3 * c + 3], raw[3 * c + 3],
                             raw[3 * c + 4])


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def class_ids(target: torch.Tensor) -> torch.Tensor:
    """The target as the kernels read it: int32; another integer type or a float type is converted with one ``.to(torch.int32)``."""
    if not isinstance(target, torch.Tensor):
        raise TypeError(f"micro_sam_amd: target must be a torch.Tensor, got {type(target).__name__}")
    if target.dtype == torch.bool or target.is_complex():
        raise TypeError(f"micro_sam_amd: target must hold class ids (an integer or floating type), got {target.dtype}")
    return target if target.dtype == torch.int32 else target.to(torch.int32)


def _operands(logits, target, dice_weight, ce_weight, softmax) -> Tuple[torch.device, int, int, int, torch.Tensor]:
    """The checks both directions share -> (device, B, C, HW, the int32 target [B, H, W])."""
    from . import ops
    dev = ops._home("logits", logits)
    ops._t("logits", logits, torch.float32, (None, None, None, None), dev)
    b, c, h, w = (int(v) for v in logits.shape)
    ops._need(2 <= c <= SEMLOSS_MAX_CLASSES, f"logits must hold 2 to {SEMLOSS_MAX_CLASSES} classes, got {list(logits.shape)}")
    ops._need(b >= 1 and h * w >= 1 and b * c * h * w < 2 ** 31, f"logits must be [B >= 1, C, H, W] with 1 <= B C H W < 2^31, got {list(logits.shape)}")
    if not isinstance(target, torch.Tensor):
        raise TypeError(f"micro_sam_amd: target must be a torch.Tensor, got {type(target).__name__}")
    ops._need(tuple(target.shape) in ((b, h, w), (b, 1, h, w)), f"target must have shape {[b, h, w]} or {[b, 1, h, w]}, got {list(target.shape)}")
    ops._need(target.device == dev, f"target lives on {target.device}, the other tensors of the call on {dev}")
    ops._need(target.is_contiguous(), f"target must be contiguous, got shape {list(target.shape)} with strides {target.stride()}")
    for name, v in (("dice_weight", dice_weight), ("ce_weight", ce_weight)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"micro_sam_amd: {name} must be a number, got {type(v).__name__}")
        ops._need(v == v and abs(v) != float("inf"), f"{name} must be finite, got {v}")
    ops._need(bool(softmax) or ce_weight == 0, "the cross-entropy needs the soft-max: softmax=False takes ce_weight=0 only")
    return dev, b, c, h * w, class_ids(target).view(b, h, w)


def semantic_loss(logits: torch.Tensor, target: torch.Tensor, dice_weight: float = 1.0, ce_weight: float = 1.0,
                  softmax: bool = True) -> Tuple[torch.Tensor, SemanticLossStats]:
    """``dice_weight * dice + ce_weight * ce`` on the device in two launches (msam_semantic_loss_forward): logits float32 [B, C, H, W],
    contiguous, 2 <= C <= 32; target [B, H, W] or [B, 1, H, W] class ids (int32; another integer type or a float type is converted once).
    dice: torch_em's ``DiceLoss()`` of ``softmax(logits, 1)`` (``softmax=False``: of the logits themselves; then ``ce_weight`` must be 0)
    against the one-hot target, summed over the classes; ce: ``nn.CrossEntropyLoss()``.  Ids outside [0, C) - -100 and every other - are
    ignored by the cross-entropy and have an all-zero one-hot; with no valid pixel ce is 0.  -> (loss: float32 0-dim,
    ``SemanticLossStats``).  Two calls agree bit for bit; nothing is read back to the host."""
    dev, b, c, hw, tgt = _operands(logits, target, dice_weight, ce_weight, softmax)
    lib = _lib.load()
    need = int(lib.msam_semantic_loss_workspace_bytes(b, c, hw))
    ws = _workspace(dev, need)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    raw = torch.empty(3 * c + 5, dtype=torch.int64, device=dev)
    _lib.check(lib.msam_semantic_loss_forward(logits.data_ptr(), tgt.data_ptr(), b, c, hw, float(dice_weight), float(ce_weight),
                                              int(bool(softmax)), SEMLOSS_EPS, ws.data_ptr(), ws.numel(), loss.data_ptr(), raw.data_ptr(),
                                              _lib.stream_ptr()), "msam_semantic_loss_forward")
    return loss, stats_views(raw, c)


def semantic_loss_backward(logits: torch.Tensor, target: torch.Tensor, stats: SemanticLossStats, grad_output: torch.Tensor,
                           dice_weight: float = 1.0, ce_weight: float = 1.0, softmax: bool = True) -> torch.Tensor:
    """d loss / d logits times ``grad_output`` (float32, one element, read on the device) in one launch (msam_semantic_loss_backward);
    ``stats`` from ``semantic_loss`` with the same arguments."""
    from . import ops
    dev, b, c, hw, tgt = _operands(logits, target, dice_weight, ce_weight, softmax)
    raw = stats.raw if isinstance(stats, SemanticLossStats) else stats
    ops._t("stats", raw, torch.int64, (3 * c + 5,), dev)
    ops._t("grad_output", grad_output, torch.float32, None, dev)
    ops._need(grad_output.numel() == 1, f"grad_output must hold one element, got shape {list(grad_output.shape)}")
    dlogits = torch.empty_like(logits)
    _lib.check(_lib.load().msam_semantic_loss_backward(logits.data_ptr(), tgt.data_ptr(), b, c, hw, float(dice_weight), float(ce_weight),
                                                       int(bool(softmax)), SEMLOSS_EPS, raw.data_ptr(), grad_output.data_ptr(),
                                                       dlogits.data_ptr(), _lib.stream_ptr()), "msam_semantic_loss_backward")
    return dlogits
