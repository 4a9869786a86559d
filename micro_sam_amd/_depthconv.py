"""``ops.depth_conv3``: the Python side of csrc/depthconv.hip (msam_depth_conv3_bf16), the depth convolution of the 3-d adapter
(``models.sam_3d_wrapper.NDBlockWrapper``) on token-major rows.  Defined here and re-exported by micro_sam_amd/ops.py with the boundary
checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); every check runs before the launch.
tests/test_depth_conv_host.py and tests/test_gpu_depth_conv.py run it."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib


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
    from . import ops
    dev = ops._home("x16", x16)
    for name, v in (("B", B), ("D", D), ("T", T)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"micro_sam_amd: {name} must be an int, got {type(v).__name__}")
        ops._need(v >= 1, f"{name} must be at least 1, got {v}")
    ops._t("x16", x16, torch.bfloat16, (B * D * T, None), dev, rows=True)
    m, ci = (int(v) for v in x16.shape)
    ops._need(ci >= 64 and ci % 64 == 0, f"x16 must hold a positive multiple of 64 channels, got {list(x16.shape)}")
    ops._t("w16", w16, torch.bfloat16, (None, 3 * ci), dev)
    co = int(w16.shape[0])
    ops._need(co >= 128 and co % 128 == 0, f"w16 must hold a positive multiple of 128 rows, got {list(w16.shape)}")
    ldx = int(x16.stride(0)) if m > 1 else ci
    ops._need(ldx % 8 == 0 and x16.data_ptr() % 16 == 0 and w16.data_ptr() % 16 == 0,
              f"x16 and w16 must be 16-byte aligned with a row stride in eights, got a stride of {ldx}")
    ops._need(m * ldx * 2 < 2 ** 31 and co * 3 * ci * 2 < 2 ** 31, f"x16 and w16 must stay below 2^31 bytes, got {m} rows of {ldx}")
    bias_ptr = ops._opt("bias", bias, torch.float32, (co,), dev)
    ops._need(bias is None or bias_ptr % 16 == 0, "bias must be 16-byte aligned")
    if out is None:
        out = torch.empty((m, co), dtype=torch.float32, device=dev)
    ops._t("out", out, torch.float32, (m, co), dev)
    ops._need(out.data_ptr() % 16 == 0, "out must be 16-byte aligned")
    _lib.check(_lib.load().msam_depth_conv3_bf16(x16.data_ptr(), ldx, w16.data_ptr(), bias_ptr, out.data_ptr(), co, B, D, T, ci, co,
                                                 _lib.stream_ptr()), "msam_depth_conv3_bf16")
    return out
