"""``ops.depth_conv3``: the Python side of msam_depth_conv3_bf16 (csrc/conv3d.hip, the depth geometry of its tile body), the depth
convolution of the 3-d adapter (``models.sam_3d_wrapper.NDBlockWrapper``) on token-major rows.  Defined here and re-exported by
micro_sam_amd/ops.py; it states its own shape rules and shares every other boundary check with ``ops.conv3d_k3``
(``_conv3d._forward_operands``); every check runs before the launch.
tests/test_depth_conv_host.py and tests/test_gpu_depth_conv.py run it."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._conv3d import _forward_operands


def tap_major(weight: torch.Tensor) -> torch.Tensor:
    """``Conv3d(Ci, Co, (3, 1, 1)).weight`` [Co, Ci, 3, 1, 1] -> [Co, 3 Ci] with columns j Ci .. (j + 1) Ci - 1 = tap j (same dtype)."""
    co, ci = weight.shape[:2]
    return weight.reshape(co, ci, 3).permute(0, 2, 1).reshape(co, 3 * ci).contiguous()


def tap_major_transposed(weight: torch.Tensor) -> torch.Tensor:
    """The operand of the input gradient, dX = conv(dY, W'): [Ci, 3 Co] with W'[ci, j Co + co] = weight[co, ci, 2 - j]."""
    co, ci = weight.shape[:2]
    return weight.reshape(co, ci, 3).flip(2).permute(1, 2, 0).reshape(ci, 3 * co).contiguous()


def depth_conv3(x16: torch.Tensor, w16: torch.Tensor, bias: Optional[torch.Tensor], B: int, D: int, T: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, z, t, :] = bias + sum_j W_j x[b, z + j - 1, t, :] over the slices inside the volume, in one launch (msam_depth_conv3_bf16):
    ``x16`` bf16 [B D T, Ci] with contiguous rows, ``w16`` bf16 [Co, 3 Ci] tap-major (``tap_major``), ``bias`` fp32 [Co] or None ->
    fp32 [B D T, Co] (``out``: written in place).  Ci % 64 == 0, Co % 128 == 0; T is arbitrary.  Two calls agree bit for bit."""
    ldx, ci, co, bias_ptr, out = _forward_operands(x16, w16, bias, out, dims=dict(B=B, D=D, T=T),
                                                   ci_ok=lambda c: c >= 64 and c % 64 == 0,
                                                   ci_text="a positive multiple of 64 channels", row_len=lambda c: 3 * c, co_step=128)
    _lib.check(_lib.load().msam_depth_conv3_bf16(x16.data_ptr(), ldx, w16.data_ptr(), bias_ptr, out.data_ptr(), co, B, D, T, ci, co,
                                                 _lib.stream_ptr()), "msam_depth_conv3_bf16")
    return out
