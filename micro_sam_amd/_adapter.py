"""``ops.adapter_``: the Python side of msam_adapter_bf16 (csrc/adapter.hip), the AdaptFormer branch of an image-encoder block
(``models.peft_sam.AdaptFormer``) as one launch.  Defined here and re-exported by micro_sam_amd/ops.py, like the other kernel families;
every check runs before the launch.  tests/test_adapter_host.py runs the kernel on the host, tests/test_gpu_adapter.py on the device,
tests/test_adapter_boundary_host.py the checks below."""
from __future__ import annotations

import torch

from . import _lib
from .ops import _code, _home, _need, _t

_F32 = torch.float32
_16 = (torch.bfloat16, torch.float16)


def adapter_(x: torch.Tensor, y: torch.Tensor, wd: torch.Tensor, bd: torch.Tensor, wu: torch.Tensor, bu: torch.Tensor,
             alpha: torch.Tensor) -> torch.Tensor:
    """``x += y + alpha * (relu(y @ wd.T + bd) @ wu.T + bu)`` in place, in one launch: ``x`` fp32 [R, D] (the residual stream), ``y``
    bf16 or fp16 [R, D] (the block's norm2 output), ``wd`` [P, D] and ``wu`` [D, P] of y's type, ``bd`` fp32 [P], ``bu`` fp32 [D], ``alpha``
    fp32 [1] on the device (no host synchronisation).  ``x`` and ``y`` may be 2-d views with contiguous rows.  D % 128 == 0, P a multiple
    of 32 in 32 .. 128.  fp32 accumulation; the hidden is rounded once to y's type and stays on the chip.  Returns ``x``."""
    dev = _home("x", x)
    _t("x", x, _F32, (None, None), dev, rows=True)
    R, D = x.shape
    _need(R >= 1 and D >= 128 and D % 128 == 0, f"x must hold R >= 1 rows of D = a positive multiple of 128 columns, got {list(x.shape)}")
    _t("y", y, _16, (R, D), dev, rows=True)
    _t("wd", wd, y.dtype, (None, D), dev)
    P = wd.shape[0]
    _need(32 <= P <= 128 and P % 32 == 0, f"wd must have P = a multiple of 32 in 32 .. 128 rows, got {P}")
    _t("bd", bd, _F32, (P,), dev)
    _t("wu", wu, y.dtype, (D, P), dev)
    _t("bu", bu, _F32, (D,), dev)
    _t("alpha", alpha, _F32, (1,), dev)
    ldy = y.stride(0) if R > 1 else D
    ldx = x.stride(0) if R > 1 else D
    _need(ldy % 8 == 0 and y.data_ptr() % 16 == 0, f"y must start on a 16-byte boundary with a row stride in eights, got a stride of {ldy}")
    _need(wd.data_ptr() % 16 == 0 and wu.data_ptr() % 16 == 0, "wd and wu must start on a 16-byte boundary")
    _lib.check(_lib.load().msam_adapter_bf16(y.data_ptr(), ldy, wd.data_ptr(), bd.data_ptr(), wu.data_ptr(), bu.data_ptr(), alpha.data_ptr(),
                                             x.data_ptr(), ldx, R, D, P, _code("y", y.dtype), _lib.stream_ptr()), "msam_adapter_bf16")
    return x
