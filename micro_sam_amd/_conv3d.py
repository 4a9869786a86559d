"""``ops.conv3d_k3``, ``ops.conv3d_k3_wgrad``, ``ops.instance_norm_stats``, ``ops.instance_norm_apply``, ``ops.instance_norm_backward`` and
``ops.column_sums``: the Python side of csrc/conv3d.hip, the 3 x 3 x 3 convolution and the InstanceNorm of the volumetric convolutional
decoder (``models.simple_sam_3d_wrapper``) on channels-last voxel rows [B D H W, C]; ``_forward_operands`` also serves the file's other
forward entry, ``_depthconv.depth_conv3``.  Defined here and re-exported by micro_sam_amd/ops.py
with the boundary checks of the other wrappers (``ops._home`` / ``ops._t`` / ``ops._need``); every check runs before the launch.
tests/test_conv3d_host.py, tests/test_gpu_conv3d.py, tests/test_instnorm_host.py and tests/test_gpu_instnorm.py run them."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

INSTANCE_NORM_EPS = 1e-5                 # torch.nn.InstanceNorm3d's default
LEAKY_SLOPE = 0.01                       # torch.nn.LeakyReLU's default


def padded_k(ci: int) -> int:
    """27 Ci rounded up to the kernel's k-tile of 64."""
    return (27 * ci + 63) // 64 * 64


def padded_co(co: int) -> int:
    """Output channels rounded up to the narrowest N tile (16): at most twice the real ones for Co >= 8."""
    return (co + 15) // 16 * 16


def tap_major(weight: torch.Tensor) -> torch.Tensor:
    """``Conv3d(Ci, Co, 3).weight`` [Co, Ci, 3, 3, 3] -> the kernel's operand [Co', Kp]: column ((kz 3 + ky) 3 + kx) Ci + ci, zero columns
    up to ``padded_k(Ci)`` and zero rows up to ``padded_co(Co)`` (same dtype)."""
    co, ci = int(weight.shape[0]), int(weight.shape[1])
    out = weight.new_zeros((padded_co(co), padded_k(ci)))
    out[:co, :27 * ci] = weight.reshape(co, ci, 27).permute(0, 2, 1).reshape(co, 27 * ci)
    return out


def tap_major_transposed(weight: torch.Tensor) -> torch.Tensor:
    """The operand of the input gradient, dX = conv(dY, W'): [Ci', Kp(Co)] with W'[ci, tap Co + co] = weight[co, ci, 26 - tap]."""
    co, ci = int(weight.shape[0]), int(weight.shape[1])
    out = weight.new_zeros((padded_co(ci), padded_k(co)))
    out[:ci, :27 * co] = weight.reshape(co, ci, 27).flip(2).permute(1, 2, 0).reshape(ci, 27 * co)
    return out


def _dims(**dims) -> None:
    from . import ops
    for name, v in dims.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"micro_sam_amd: {name} must be an int, got {type(v).__name__}")
        ops._need(v >= 1, f"{name} must be at least 1, got {v}")


def _stride(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _forward_operands(x16, w16, bias, out, *, dims: dict, ci_ok, ci_text: str, row_len, co_step: int):
    """The checks ``conv3d_k3`` and ``depth_conv3`` share, in their order: the device, the int dims (their product is the number of rows),
    the bf16 rows, the channels (``ci_ok`` / ``ci_text``: the caller's rule), the weight [a positive multiple of ``co_step``,
    ``row_len(Ci)``], alignment, the byte limits, the optional bias and the optional ``out`` -> (ldx, Ci, Co, the bias pointer, out)."""
    from . import ops
    dev = ops._home("x16", x16)
    _dims(**dims)
    rows = 1
    for v in dims.values():
        rows *= v
    ops._t("x16", x16, torch.bfloat16, (rows, None), dev, rows=True)
    m, ci = (int(v) for v in x16.shape)
    ops._need(ci_ok(ci), f"x16 must hold {ci_text}, got {list(x16.shape)}")
    ops._t("w16", w16, torch.bfloat16, (None, row_len(ci)), dev)
    co = int(w16.shape[0])
    ops._need(co >= co_step and co % co_step == 0, f"w16 must hold a positive multiple of {co_step} rows, got {list(w16.shape)}")
    ldx = _stride(x16)
    ops._need(ldx % 8 == 0 and x16.data_ptr() % 16 == 0 and w16.data_ptr() % 16 == 0,
              f"x16 and w16 must be 16-byte aligned with a row stride in eights, got a stride of {ldx}")
    ops._need(m * ldx * 2 < 2 ** 31 and co * row_len(ci) * 2 < 2 ** 31, f"x16 and w16 must stay below 2^31 bytes, got {m} rows of {ldx}")
    bias_ptr = ops._opt("bias", bias, torch.float32, (co,), dev)
    ops._need(bias is None or bias_ptr % 16 == 0, "bias must be 16-byte aligned")
    if out is None:
        out = torch.empty((m, co), dtype=torch.float32, device=dev)
    ops._t("out", out, torch.float32, (m, co), dev)
    ops._need(out.data_ptr() % 16 == 0, "out must be 16-byte aligned")
    return ldx, ci, co, bias_ptr, out


def conv3d_k3(x16: torch.Tensor, w16: torch.Tensor, bias: Optional[torch.Tensor], B: int, D: int, H: int, W: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Conv3d(Ci, Co, 3, padding=1)`` in one launch (msam_conv3d_k3_bf16): ``x16`` bf16 [B D H W, Ci] with contiguous rows (a row
    stride in eights), ``w16`` bf16 [Co', padded_k(Ci)] (``tap_major``), ``bias`` fp32 [Co'] or None -> fp32 [B D H W, Co'] (``out``:
    written in place).  Ci % 8 == 0, Co' % 16 == 0.  Two calls agree bit for bit."""
    ldx, ci, co, bias_ptr, out = _forward_operands(x16, w16, bias, out, dims=dict(B=B, D=D, H=H, W=W),
                                                   ci_ok=lambda c: 8 <= c <= 4096 and c % 8 == 0,
                                                   ci_text="a multiple of 8 channels in 8 .. 4096", row_len=padded_k, co_step=16)
    _lib.check(_lib.load().msam_conv3d_k3_bf16(x16.data_ptr(), ldx, w16.data_ptr(), bias_ptr, out.data_ptr(), co, B, D, H, W, ci, co,
                                               _lib.stream_ptr()), "msam_conv3d_k3_bf16")
    return out


def conv3d_k3_wgrad(x16: torch.Tensor, dy16: torch.Tensor, B: int, D: int, H: int, W: int) -> torch.Tensor:
    """The weight gradient of ``conv3d_k3`` (msam_conv3d_k3_wgrad_bf16): ``x16`` bf16 [M, Ci], ``dy16`` bf16 [M, Co] (row strides in
    eights, Ci and Co multiples of 8) -> fp32 [Co, Ci, 3, 3, 3].  Split over the voxels, the parts added in split order."""
    from . import ops
    dev = ops._home("x16", x16)
    _dims(B=B, D=D, H=H, W=W)
    m = B * D * H * W
    ops._t("x16", x16, torch.bfloat16, (m, None), dev, rows=True)
    ops._t("dy16", dy16, torch.bfloat16, (m, None), dev, rows=True)
    ci, co = int(x16.shape[1]), int(dy16.shape[1])
    ops._need(8 <= ci <= 4096 and ci % 8 == 0 and co >= 8 and co % 8 == 0 and 27 * ci * co < 2 ** 28,
              f"x16 and dy16 must hold multiples of 8 channels (x16 at most 4096), got {ci} and {co}")
    ldx, ldy = _stride(x16), _stride(dy16)
    ops._need(ldx % 8 == 0 and ldy % 8 == 0 and x16.data_ptr() % 16 == 0 and dy16.data_ptr() % 16 == 0,
              f"x16 and dy16 must be 16-byte aligned with row strides in eights, got {ldx} and {ldy}")
    ops._need(m * ldx * 2 < 2 ** 31 and m * ldy * 2 < 2 ** 31, f"x16 and dy16 must stay below 2^31 bytes, got {m} rows of {ldx} and {ldy}")
    lib = _lib.load()
    need = int(lib.msam_conv3d_k3_wgrad_workspace_bytes(B, D, H, W, ci, co))
    ops._need(need > 0, "msam_conv3d_k3_wgrad_workspace_bytes refused the shape")
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    dw = torch.empty((27 * ci, co), dtype=torch.float32, device=dev)
    _lib.check(lib.msam_conv3d_k3_wgrad_bf16(x16.data_ptr(), ldx, dy16.data_ptr(), ldy, dw.data_ptr(), ws.data_ptr(), need, B, D, H, W, ci,
                                             co, _lib.stream_ptr()), "msam_conv3d_k3_wgrad_bf16")
    return dw.reshape(27, ci, co).permute(2, 1, 0).reshape(co, ci, 3, 3, 3).contiguous()


def _rows32(name: str, t, m: int, c: int, dev) -> int:
    """An fp32 row matrix [m, c] with contiguous rows, a stride in fours and a 16-byte aligned base -> its row stride."""
    from . import ops
    ops._t(name, t, torch.float32, (m, c), dev, rows=True)
    ld = _stride(t)
    ops._need(ld % 4 == 0 and t.data_ptr() % 16 == 0, f"{name} must be 16-byte aligned with a row stride in fours, got {ld}")
    return ld


def _in_shape(a: torch.Tensor, B: int, V: int) -> Tuple[torch.device, int, int]:
    from . import ops
    dev = ops._home("a", a)
    _dims(B=B, V=V)
    if V < 2:
        raise ValueError(f"micro_sam_amd: InstanceNorm expects more than 1 value per channel, got V = {V}")
    ops._need(a.dim() == 2, f"a must be [B V, C], got {list(a.shape)}")
    c = int(a.shape[1])
    ops._need(4 <= c <= 1024 and c & (c - 1) == 0, f"a must hold a power of two of channels in 4 .. 1024, got {c}")
    ops._need(B * V < 2 ** 31, f"B V must stay below 2^31, got {B * V}")
    return dev, B * V, c


def _workspace(B: int, V: int, c: int, dev) -> torch.Tensor:
    need = int(_lib.load().msam_instance_norm_workspace_bytes(B, V, c))
    if need <= 0:
        raise ValueError(f"micro_sam_amd: msam_instance_norm_workspace_bytes refused B = {B}, V = {V}, C = {c}")
    return torch.empty((need,), dtype=torch.uint8, device=dev)


def _stats(name: str, t, B: int, c: int, dev) -> int:
    from . import ops
    return ops._t(name, t, torch.float64, (B, c, 2), dev).data_ptr()


def instance_norm_stats(a: torch.Tensor, B: int, V: int) -> torch.Tensor:
    """Mean and biased variance per (volume, channel) of fp32 rows [B V, C] -> fp64 [B, C, 2] (msam_instance_norm_stats: fp64 partial
    sums per workgroup, added in index order).  V < 2 raises ``ValueError``, as ``torch.nn.functional.instance_norm`` does."""
    dev, m, c = _in_shape(a, B, V)
    lda = _rows32("a", a, m, c, dev)
    ws = _workspace(B, V, c, dev)
    stats = torch.empty((B, c, 2), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().msam_instance_norm_stats(a.data_ptr(), lda, B, V, c, stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    _lib.stream_ptr()), "msam_instance_norm_stats")
    return stats


def instance_norm_apply(a: torch.Tensor, stats_a: torch.Tensor, B: int, V: int, residual: Optional[torch.Tensor] = None,
                        stats_r: Optional[torch.Tensor] = None, negative_slope: Optional[float] = LEAKY_SLOPE,
                        eps: float = INSTANCE_NORM_EPS, want32: bool = True, want16: bool = False):
    """y = leaky_relu((a - mean_a) rstd_a [+ (r - mean_r) rstd_r], negative_slope) in one pass (msam_instance_norm_apply); the residual
    term and the activation (``negative_slope`` None: none) are optional -> (fp32 [B V, C] | None, bf16 [B V, C] | None)."""
    from . import ops
    dev, m, c = _in_shape(a, B, V)
    lda = _rows32("a", a, m, c, dev)
    sa = _stats("stats_a", stats_a, B, c, dev)
    ops._need((residual is None) == (stats_r is None), "residual and stats_r come together")
    ops._need(want32 or want16, "one of want32 / want16 must be set")
    ops._need(eps >= 0, f"eps must not be negative, got {eps}")
    r_ptr, ldr, sr = None, 0, None
    if residual is not None:
        ldr = _rows32("residual", residual, m, c, dev)
        r_ptr, sr = residual.data_ptr(), _stats("stats_r", stats_r, B, c, dev)
    o32 = torch.empty((m, c), dtype=torch.float32, device=dev) if want32 else None
    o16 = torch.empty((m, c), dtype=torch.bfloat16, device=dev) if want16 else None
    _lib.check(_lib.load().msam_instance_norm_apply(a.data_ptr(), lda, sa, r_ptr, ldr, sr, B, V, c, float(eps),
                                                    float(negative_slope or 0.0), int(negative_slope is not None),
                                                    None if o32 is None else o32.data_ptr(), c, None if o16 is None else o16.data_ptr(), c,
                                                    _lib.stream_ptr()), "msam_instance_norm_apply")
    return o32, o16


def instance_norm_backward(dy: torch.Tensor, a: torch.Tensor, stats_a: torch.Tensor, B: int, V: int,
                           residual: Optional[torch.Tensor] = None, stats_r: Optional[torch.Tensor] = None,
                           negative_slope: Optional[float] = LEAKY_SLOPE, eps: float = INSTANCE_NORM_EPS):
    """The gradients of ``instance_norm_apply`` with respect to ``a`` and ``residual`` (msam_instance_norm_backward: one statistics pass,
    one elementwise pass) -> (da, dr | None), fp32 [B V, C]."""
    from . import ops
    dev, m, c = _in_shape(a, B, V)
    lda = _rows32("a", a, m, c, dev)
    ldy = _rows32("dy", dy, m, c, dev)
    sa = _stats("stats_a", stats_a, B, c, dev)
    ops._need((residual is None) == (stats_r is None), "residual and stats_r come together")
    r_ptr, ldr, sr, dr = None, 0, None, None
    if residual is not None:
        ldr = _rows32("residual", residual, m, c, dev)
        r_ptr, sr = residual.data_ptr(), _stats("stats_r", stats_r, B, c, dev)
        dr = torch.empty((m, c), dtype=torch.float32, device=dev)
    da = torch.empty((m, c), dtype=torch.float32, device=dev)
    sums = torch.empty((B, c, 3), dtype=torch.float64, device=dev)
    ws = _workspace(B, V, c, dev)
    _lib.check(_lib.load().msam_instance_norm_backward(dy.data_ptr(), ldy, a.data_ptr(), lda, sa, r_ptr, ldr, sr, B, V, c, float(eps),
                                                       float(negative_slope or 0.0), int(negative_slope is not None), da.data_ptr(), c,
                                                       None if dr is None else dr.data_ptr(), c, sums.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _lib.stream_ptr()), "msam_instance_norm_backward")
    return da, dr


def column_sums(x: torch.Tensor) -> torch.Tensor:
    """sum over the rows of fp32 [M, C] (C a power of two in 4 .. 1024) -> fp32 [C]: fp64 partial sums per workgroup, added in index order
    (msam_column_sums_f32) - the bias gradient of the convolution."""
    from . import ops
    dev = ops._home("x", x)
    ops._need(x.dim() == 2 and x.shape[0] >= 1, f"x must be [M, C], got {list(x.shape)}")
    m, c = int(x.shape[0]), int(x.shape[1])
    ops._need(4 <= c <= 1024 and c & (c - 1) == 0, f"x must hold a power of two of channels in 4 .. 1024, got {c}")
    ldx = _rows32("x", x, m, c, dev)
    ws = _workspace(1, m, c, dev)
    sums = torch.empty((c,), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().msam_column_sums_f32(x.data_ptr(), ldx, m, c, sums.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "msam_column_sums_f32")
    return sums.to(torch.float32)
