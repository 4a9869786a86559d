"""The loss of semantic-segmentation fine-tuning restated with torch operators as the reference writes it
(micro_sam/training/semantic_sam_trainer.py: ``CustomDiceLoss`` = soft-max, a per-class ``==`` and ``cat`` for the one-hot, torch_em's
``DiceLoss()`` - per channel 1 - 2 sum(p t) / clamp(sum(p^2) + sum(t^2), 1e-7), summed over the channels - plus ``nn.CrossEntropyLoss()``),
the case table of tests/test_semantic_loss_host.py and tests/test_gpu_semantic_loss.py, and the bound both use.

``composite`` runs in the dtype of its logits: in float64 it is the restatement the kernels are compared with, in float32 it is the
yardstick - what a user runs without the fused kernel.  The two documented differences of the kernel from torch are restated here, so that
the composite is defined on every case: an id outside [0, C) other than -100 is given to ``cross_entropy`` as -100 (torch raises there), and
without any valid pixel the cross-entropy is 0 (torch: NaN).

The bound: the error of the fp32 composite against the fp64 one on the same input, times 4 (the allowance of
tests/test_gpu_visualization.py: the kernel rounds in another, not a worse, order), with a floor of 2 fp32 ulps of the loss and of
2^-22 max|gradient| for every gradient entry - about a dozen fp32 roundings lie between the logits and an output."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-7


def one_hot(target: torch.Tensor, num_classes: int) -> torch.Tensor:
    """The reference's ``_one_hot_encoder``: target [B, 1, H, W] -> [B, C, H, W]; an id outside [0, C) gives zeros."""
    return torch.cat([target == i for i in range(num_classes)], dim=1)


def dice(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """torch_em ``DiceLoss()`` (channelwise, reduce_channel="sum", eps=1e-7)."""
    c = pred.shape[1]
    p = pred.transpose(0, 1).reshape(c, -1)
    t = target.transpose(0, 1).reshape(c, -1)
    num = (p * t).sum(-1)
    den = (p * p).sum(-1) + (t * t).sum(-1)
    return (1.0 - 2.0 * num / den.clamp(min=EPS)).sum()


def composite(logits: torch.Tensor, target: torch.Tensor, dice_weight=1.0, ce_weight=1.0, softmax=True):
    """logits [B, C, H, W] (float32 or float64), target int64 [B, H, W] -> (loss, dice, ce), 0-dim tensors of the logits' dtype."""
    c = logits.shape[1]
    pred = torch.softmax(logits, dim=1) if softmax else logits
    d = dice(pred, one_hot(target[:, None], c).to(logits.dtype))
    valid = (target >= 0) & (target < c)
    if softmax and bool(valid.any()):
        ce = F.cross_entropy(logits, torch.where(valid, target, torch.full_like(target, -100)))
    else:
        ce = logits.sum() * 0.0
    return dice_weight * d + ce_weight * ce, d, ce


def loss_and_gradient(logits: np.ndarray, target: np.ndarray, dtype, dice_weight=1.0, ce_weight=1.0, softmax=True, device="cpu"):
    """-> dict(loss, dice, ce: float; grad: float64 array) of the composite evaluated in ``dtype``."""
    x = torch.as_tensor(logits, device=device).to(dtype).requires_grad_()
    t = torch.as_tensor(target.astype(np.int64), device=device)
    loss, d, ce = composite(x, t, dice_weight, ce_weight, softmax)
    loss.backward()
    return {"loss": float(loss.detach().double()), "dice": float(d.detach().double()), "ce": float(ce.detach().double()),
            "grad": x.grad.double().cpu().numpy()}


def counts(target: np.ndarray, num_classes: int):
    """-> (pixels per class int64 [C], valid pixels, ignored pixels)."""
    per_class = np.array([(target == c).sum() for c in range(num_classes)], np.int64)
    valid = int(((target >= 0) & (target < num_classes)).sum())
    return per_class, valid, int(target.size - valid)


def bounds(want64: dict, yard32: dict):
    """-> (bound on |loss - loss64|, bound on every |grad - grad64|, the yardstick's own two errors)."""
    err_loss = abs(yard32["loss"] - want64["loss"])
    err_grad = float(np.abs(yard32["grad"] - want64["grad"]).max())
    floor_loss = 2.0 * float(np.spacing(np.float32(abs(want64["loss"]))))
    floor_grad = 2.0 ** -22 * float(np.abs(want64["grad"]).max())
    return max(4.0 * err_loss, floor_loss), max(4.0 * err_grad, floor_grad), err_loss, err_grad


def _case(shape, seed, scale=1.0, softmax=True, dice_weight=1.0, ce_weight=1.0, edit=None):
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    logits = (scale * rng.standard_normal(shape)).astype(np.float32)
    target = rng.integers(0, c, (b, h, w)).astype(np.int32)
    if edit is not None:
        edit(logits, target, rng)
    return {"logits": logits, "target": target, "softmax": softmax, "dice_weight": dice_weight, "ce_weight": ce_weight}


def _ragged(logits, target, rng):
    c = logits.shape[1]
    target[0, 5, :] = -100                                              # a row of torch's ignore_index
    target[1, 0, :3] = c                                                # ids just outside the range on both sides
    target[1, 7, 11:14] = -1
    target[0, 32, 64] = 1000


def _never(logits, target, rng):
    target[target == 4] = 0                                             # class 4 never occurs


def _runtime(logits, target, rng):
    target[0, 2, :] = -100
    target[0, 3, 1] = 9
    target[target == 7] = 3                                             # class 7 never occurs


def _no_valid(logits, target, rng):
    target[:] = -100
    target[0, 1, :4] = 3
    target[0, 2, :4] = -1


def _pm80(logits, target, rng):
    logits[:] = np.where(rng.random(logits.shape) < 0.5, -80.0, 80.0).astype(np.float32)


def _zero_channel(logits, target, rng):
    logits[:, 1] = 0.0                                                  # den_1 = 0: that class's term is 1, its gradient 0
    target[target == 1] = 2


def cases():
    """name -> dict(logits float32 [B, C, H, W], target int32 [B, H, W], softmax, dice_weight, ce_weight): the smallest shapes at which
    the kernels take another path - less than a wave; ragged (HW % 4 != 0: one pixel per thread); four pixels per thread; 5, 6 and 8
    classes in registers; 9 and 32 classes in the run-time loops; more than one workgroup (2048 pixels each); more than 256 workgroups, so that
    a thread of the last stage adds several partials."""
    return {
        "7x9_c2": _case((1, 2, 7, 9), 1),
        "33x65_c3_ignored": _case((2, 3, 33, 65), 2, edit=_ragged),
        "64x64_c3": _case((2, 3, 64, 64), 3),
        "16x16_c5_never": _case((2, 5, 16, 16), 4, edit=_never),
        "8x8_c6_weights": _case((1, 6, 8, 8), 5, dice_weight=0.3, ce_weight=0.7),
        "9x7_c8": _case((1, 8, 9, 7), 6),
        "8x8_c9_runtime": _case((1, 9, 8, 8), 7, edit=_runtime),
        "5x5_c32_runtime": _case((1, 32, 5, 5), 8),
        "12x12_c12_runtime_vec": _case((2, 12, 12, 12), 9, scale=3.0),
        "192x192_c3_scaled": _case((2, 3, 192, 192), 10, scale=3.0),
        "513x1024_c2_many_partials": _case((1, 2, 513, 1024), 16),
        "8x8_c3_no_valid": _case((1, 3, 8, 8), 11, edit=_no_valid),
        "16x16_c3_pm80": _case((1, 3, 16, 16), 12, edit=_pm80),
        "16x16_c3_raw_zero_channel": _case((2, 3, 16, 16), 13, softmax=False, ce_weight=0.0, edit=_zero_channel),
        "16x15_c4_dice_only": _case((1, 4, 16, 15), 14, ce_weight=0.0),
        "16x16_c10_raw_runtime": _case((1, 10, 16, 16), 15, softmax=False, ce_weight=0.0),
    }


_REF = {}


def reference(name: str):
    """(fp64 restatement, fp32 yardstick) of a case, computed once and shared by the tests (treat as read-only)."""
    if name not in _REF:
        k = cases()[name]
        kw = dict(dice_weight=k["dice_weight"], ce_weight=k["ce_weight"], softmax=k["softmax"])
        _REF[name] = (loss_and_gradient(k["logits"], k["target"], torch.float64, **kw),
                      loss_and_gradient(k["logits"], k["target"], torch.float32, **kw))
    return _REF[name]
